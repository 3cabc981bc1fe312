// dr_nurbs_device.hip -- Nurbs.refine (shapes/nurbs.dart:76-154) ON THE GPU: dr_nurbs_dice_device.  The refusals and the
// homogeneous control net are the host's (nb_prepare, dr_nurbs_host.cpp); the dice points and the indices are two kernels:
//   k_nurbs_dice<STAGE>  lane = dice point pi = v * diceu + u (u fastest: a wave's P / N / uv stores are three contiguous runs).  The rules
//                        are dr_nurbs.h's nb_vertex, the ones the host builder loops over.  STAGE: the two knot vectors and the control
//                        net are copied once per workgroup into LDS when they fit DR_NB_LDS_BYTES (16 KiB -- ten workgroups of it still
//                        fit a CU's 160 KiB) and every lane reads them there: the indices are wave-uniform along u for the v direction
//                        and near-uniform otherwise, so an LDS read is a broadcast.  Otherwise the same reads go to global memory
//                        through the caches.  cpWork / iso are per-lane arrays indexed by loop counters that depend on the order: see
//                        MEASUREMENTS.md for where the compiler puts them.
//   k_nurbs_indices      lane = quad: six indices (nb_quad), 24 contiguous bytes per lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "../../include/dartray_hip.h"

#include "dr_nurbs.h"
#include "dr_options.h"

namespace {

#define DR_NB_BLOCK 256
#define DR_NB_LDS_BYTES 16384
#define DR_NB_LDS_FLOATS (DR_NB_LDS_BYTES / 4)

template <bool STAGE>
__global__ void __launch_bounds__(DR_NB_BLOCK) k_nurbs_dice(NbPatch p, uint32_t nverts, float* __restrict__ P, float* __restrict__ N,
                                                            float* __restrict__ uv) {
  if (STAGE) {
    __shared__ float s_data[DR_NB_LDS_FLOATS];
    const uint32_t nuk = (uint32_t)(p.nu + p.uorder), nvk = (uint32_t)(p.nv + p.vorder), ncp = 4u * (uint32_t)p.nu * (uint32_t)p.nv;
    for (uint32_t i = threadIdx.x; i < nuk; i += DR_NB_BLOCK) s_data[i] = p.uknot[i];
    for (uint32_t i = threadIdx.x; i < nvk; i += DR_NB_BLOCK) s_data[nuk + i] = p.vknot[i];
    for (uint32_t i = threadIdx.x; i < ncp; i += DR_NB_BLOCK) s_data[nuk + nvk + i] = p.Pw[i];
    __syncthreads();
    p.uknot = s_data;
    p.vknot = s_data + nuk;
    p.Pw = s_data + nuk + nvk;
  }
  const uint32_t pi = blockIdx.x * DR_NB_BLOCK + threadIdx.x;
  if (pi >= nverts) return;
  const NbVertex o = nb_vertex(p, pi % p.diceu, pi / p.diceu);
  for (int c = 0; c < 3; ++c) {
    P[3 * (size_t)pi + c] = o.P[c];
    N[3 * (size_t)pi + c] = o.N[c];
  }
  uv[2 * (size_t)pi] = o.uv[0];
  uv[2 * (size_t)pi + 1] = o.uv[1];
}

__global__ void __launch_bounds__(DR_NB_BLOCK) k_nurbs_indices(uint32_t diceu, uint32_t nquads, uint32_t* __restrict__ indices) {
  const uint32_t q = blockIdx.x * DR_NB_BLOCK + threadIdx.x;
  if (q >= nquads) return;
  uint32_t six[6];
  nb_quad(diceu, q % (diceu - 1u), q / (diceu - 1u), six);
  for (int c = 0; c < 6; ++c) indices[6 * (size_t)q + c] = six[c];
}

template <class T>
struct Buf {
  T* p = nullptr;
  hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};
struct Event {
  hipEvent_t e = nullptr;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
};
#define ST(x)                                                                                                       \
  do {                                                                                                              \
    hipError_t e_ = (x);                                                                                            \
    if (e_ != hipSuccess) return dr_fail(DR_ERR_HIP, std::string("dr_nurbs_dice_device: ") + hipGetErrorString(e_)); \
  } while (0)

unsigned grid(uint64_t n) { return (unsigned)((n + DR_NB_BLOCK - 1) / DR_NB_BLOCK); }

}  // namespace

extern "C" int dr_nurbs_dice_device(const DrNurbsPatch* patch, float* P_out, float* N_out, float* uv_out, uint32_t* indices_out,
                                    uint64_t vert_cap, uint64_t tri_cap, uint64_t* nverts_out, uint64_t* ntris_out) {
  NbPrepared prep;
  int rc = nb_prepare("dr_nurbs_dice_device", patch, prep);
  if (rc != DR_OK) return rc;
  bool done = false;
  rc = nb_check_outputs("dr_nurbs_dice_device", prep, P_out, N_out, uv_out, indices_out, vert_cap, tri_cap, nverts_out, ntris_out, &done);
  if (rc != DR_OK || done) return rc;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, "dr_nurbs_dice_device before dr_init");
  const bool dbg = dr_opt("DARTRAY_VERBOSE").toInt(0) >= 2;
  hipStream_t s = 0;
  NbPatch p = prep.view;
  const size_t nuk = (size_t)p.nu + p.uorder, nvk = (size_t)p.nv + p.vorder, ncp = prep.Pw.size();
  const uint32_t nverts = (uint32_t)prep.nverts, nquads = (uint32_t)(prep.ntris / 2);

  Buf<float> patchData, P, N, uv;  // patchData: uknot, vknot, Pw, one upload
  Buf<uint32_t> indices;
  ST(patchData.alloc(nuk + nvk + ncp));
  ST(P.alloc(3 * (size_t)nverts));
  ST(N.alloc(3 * (size_t)nverts));
  ST(uv.alloc(2 * (size_t)nverts));
  ST(indices.alloc(6 * (size_t)nquads));
  Event e0, e1;
  ST(hipEventCreate(&e0.e));
  ST(hipEventCreate(&e1.e));
  ST(hipMemcpyAsync(patchData.p, p.uknot, nuk * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(patchData.p + nuk, p.vknot, nvk * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(patchData.p + nuk + nvk, prep.Pw.data(), ncp * sizeof(float), hipMemcpyHostToDevice, s));
  p.uknot = patchData.p;
  p.vknot = patchData.p + nuk;
  p.Pw = patchData.p + nuk + nvk;

  const bool stage = nuk + nvk + ncp <= DR_NB_LDS_FLOATS;
  ST(hipEventRecord(e0.e, s));
  if (stage)
    hipLaunchKernelGGL(k_nurbs_dice<true>, dim3(grid(nverts)), dim3(DR_NB_BLOCK), 0, s, p, nverts, P.p, N.p, uv.p);
  else
    hipLaunchKernelGGL(k_nurbs_dice<false>, dim3(grid(nverts)), dim3(DR_NB_BLOCK), 0, s, p, nverts, P.p, N.p, uv.p);
  hipLaunchKernelGGL(k_nurbs_indices, dim3(grid(nquads)), dim3(DR_NB_BLOCK), 0, s, p.diceu, nquads, indices.p);
  ST(hipGetLastError());
  ST(hipEventRecord(e1.e, s));

  ST(hipMemcpyAsync(P_out, P.p, 3 * (size_t)nverts * sizeof(float), hipMemcpyDeviceToHost, s));
  ST(hipMemcpyAsync(N_out, N.p, 3 * (size_t)nverts * sizeof(float), hipMemcpyDeviceToHost, s));
  ST(hipMemcpyAsync(uv_out, uv.p, 2 * (size_t)nverts * sizeof(float), hipMemcpyDeviceToHost, s));
  ST(hipMemcpyAsync(indices_out, indices.p, 6 * (size_t)nquads * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  ST(hipStreamSynchronize(s));
  if (dbg) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0.e, e1.e);
    fprintf(stderr, "[dartray_hip] dr_nurbs_dice_device: %u x %u points, order %d x %d, patch data in %s: %.3f ms on the device (HIP events: k_nurbs_dice and k_nurbs_indices; upload and copy-out excluded)\n",
            p.diceu, p.dicev, p.uorder, p.vorder, stage ? "LDS" : "global memory", ms);
  }
  return DR_OK;
}
