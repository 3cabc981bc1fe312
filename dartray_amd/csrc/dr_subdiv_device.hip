// dr_subdiv_device.hip -- LoopSubdivision.refine (shapes/loop_subdivision.dart:99-308) ON THE GPU: dr_loop_subdivide_device.
// Level 0 -- the constructor's topology and every refusal -- is the host's (sd_prepare, dr_subdiv_host.cpp); the levels and everything
// behind the last one run here, level after level, with the mesh resident in two sets of flat arrays that take turns:
//   k_subdiv_even                                lane = old vertex: the even child's position (one-ring / boundary rule) and flags
//   k_subdiv_edge_count / _scan / _edge_scatter  lane = (face, k) slot: does the slot create its edge's odd vertex, and which number does
//                                                it get -- order of first appearance = rank among the creating slots: wave ballots, workgroup
//                                                sums through LDS, one scan workgroup over the block sums (k_halton_count / _scan / _scatter
//                                                in shape; no atomic decides a number).  Writes edgeVert[slot] for the creating slot -- the
//                                                other side of the edge reads it through its neighbour -- and the list of creating slots
//   k_subdiv_odd                                 lane = created edge: the odd vertex's position, flags and startFace
//   k_subdiv_topology                            lane = old face: its four children's v[] / f[], the even children's startFace
// and after the last level
//   k_subdiv_limit                               lane = vertex: the limit position, read from the level's buffer, written to another
//   k_subdiv_normals                             lane = vertex: S, T from the ring's limit positions and the host's cos / sin table
// The indices are the last level's faceV as it stands, copied out.
// The per-element rules are dr_subdiv.h's, the ones the host builder loops over: the outputs are byte-identical (tests/test_gpu_subdiv.py).
// The ring walks are chains of dependent, divergent loads (face -> its three vertex numbers -> the neighbour -> ...), about a dozen
// round trips per vertex and nothing to overlap them with but other waves: latency bound, not bandwidth bound; the kernels keep their
// register use small so that every SIMD holds its full share of waves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/dartray_hip.h"

#include "dr_options.h"
#include "dr_subdiv.h"

namespace {

#define DR_SD_BLOCK 256  // lanes per workgroup of every kernel here; slots per entry of the block counts

__device__ __forceinline__ int sd_lane() { return (int)(threadIdx.x & 63); }

__global__ void __launch_bounds__(DR_SD_BLOCK) k_subdiv_even(SdMesh m, float* P2, uint8_t* flags2) {
  const uint32_t v = blockIdx.x * DR_SD_BLOCK + threadIdx.x;
  if (v >= m.nv) return;
  sd_store(P2, v, sd_even(m, (int32_t)v));
  flags2[v] = m.vertFlags[v];
}

// blk[b]: creating slots of workgroup b
__global__ void __launch_bounds__(DR_SD_BLOCK) k_subdiv_edge_count(SdMesh m, uint32_t nslots, uint32_t* blk) {
  __shared__ uint32_t s_wave[DR_SD_BLOCK / 64];
  const uint32_t slot = blockIdx.x * DR_SD_BLOCK + threadIdx.x;
  const bool c = slot < nslots && sd_creates(m, slot);
  const unsigned long long mask = __ballot(c);
  if (sd_lane() == 0) s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0u;
    for (int w = 0; w < DR_SD_BLOCK / 64; ++w) sum += s_wave[w];
    blk[blockIdx.x] = sum;
  }
}

// One workgroup: blk[0 .. nblk) becomes its exclusive prefix sum, blk[nblk] the total.  A thread owns a contiguous run of entries; the
// runs' sums are scanned inside each wave by shuffles and across the 16 waves through LDS.
__global__ void __launch_bounds__(1024) k_subdiv_scan(uint32_t* blk, uint32_t nblk) {
  __shared__ uint32_t s_wave[16];
  const uint32_t per = (nblk + 1023u) / 1024u;
  const uint32_t b0 = min(threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
  uint32_t sum = 0u;
  for (uint32_t b = b0; b < b1; ++b) sum += blk[b];
  const int lane = sd_lane(), wave = (int)(threadIdx.x >> 6);
  uint32_t inc = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, off);
    if (lane >= off) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t run = inc - sum;
  for (int w = 0; w < wave; ++w) run += s_wave[w];
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t c = blk[b];
    blk[b] = run;
    run += c;
  }
  if (threadIdx.x == 1023u) blk[nblk] = run;
}

// The test again, and every creating slot its number: the workgroup's offset + the creating slots of the waves before this one + those of
// the lower lanes of this wave.  edgeVert[slot] = the odd vertex's number in the next level, created[rank] = slot.
__global__ void __launch_bounds__(DR_SD_BLOCK) k_subdiv_edge_scatter(SdMesh m, uint32_t nslots, const uint32_t* blk, uint32_t ncreated,
                                                                     int32_t* edgeVert, uint32_t* created) {
  __shared__ uint32_t s_wave[DR_SD_BLOCK / 64];
  const uint32_t slot = blockIdx.x * DR_SD_BLOCK + threadIdx.x;
  const bool c = slot < nslots && sd_creates(m, slot);
  const unsigned long long mask = __ballot(c);
  const int lane = sd_lane(), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (!c) return;
  uint32_t at = blk[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) at += s_wave[w];
  if (at >= ncreated) return;  // (cannot happen on a validated mesh: the host sized `created` by the edge count)
  edgeVert[slot] = (int32_t)(m.nv + at);
  created[at] = slot;
}

__global__ void __launch_bounds__(DR_SD_BLOCK) k_subdiv_odd(SdMesh m, const uint32_t* created, uint32_t ncreated, float* P2, uint8_t* flags2,
                                                            int32_t* start2) {
  const uint32_t r = blockIdx.x * DR_SD_BLOCK + threadIdx.x;
  if (r >= ncreated) return;
  const uint32_t slot = created[r];
  const size_t v = (size_t)m.nv + r;
  sd_store(P2, v, sd_odd(m, slot));
  flags2[v] = (uint8_t)(DR_SD_REGULAR | (m.faceF[slot] < 0 ? DR_SD_BOUNDARY : 0u));
  start2[v] = (int32_t)(4u * (slot / 3u) + 3u);
}

__global__ void __launch_bounds__(DR_SD_BLOCK) k_subdiv_topology(SdMesh m, const int32_t* edgeVert, int32_t* faceV2, int32_t* faceF2,
                                                                 int32_t* start2) {
  const uint32_t j = blockIdx.x * DR_SD_BLOCK + threadIdx.x;
  if (j >= m.nf) return;
  sd_topology(m, edgeVert, j, faceV2, faceF2, start2);
}

__global__ void __launch_bounds__(DR_SD_BLOCK) k_subdiv_limit(SdMesh m, float* Plimit) {
  const uint32_t v = blockIdx.x * DR_SD_BLOCK + threadIdx.x;
  if (v >= m.nv) return;
  sd_store(Plimit, v, sd_limit(m, (int32_t)v));
}

// m.P: the limit positions
__global__ void __launch_bounds__(DR_SD_BLOCK) k_subdiv_normals(SdMesh m, SdTrig trig, float* N) {
  const uint32_t v = blockIdx.x * DR_SD_BLOCK + threadIdx.x;
  if (v >= m.nv) return;
  sd_store(N, v, sd_normal(m, trig, (int32_t)v));
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
#define ST(x)                                                                                                               \
  do {                                                                                                                      \
    hipError_t e_ = (x);                                                                                                    \
    if (e_ != hipSuccess) return dr_fail(DR_ERR_HIP, std::string("dr_loop_subdivide_device: ") + hipGetErrorString(e_)); \
  } while (0)

// One level's arrays in device memory
struct Level {
  Buf<int32_t> faceV, faceF, vertStart;
  Buf<uint8_t> vertFlags;
  Buf<float> P;
  hipError_t alloc(uint64_t nf, uint64_t nv) {
    hipError_t e = faceV.alloc(3 * nf);
    if (e == hipSuccess) e = faceF.alloc(3 * nf);
    if (e == hipSuccess) e = vertStart.alloc(nv);
    if (e == hipSuccess) e = vertFlags.alloc(nv);
    return e != hipSuccess ? e : P.alloc(3 * nv);
  }
  SdMesh mesh(uint64_t nf, uint64_t nv) const { return SdMesh{faceV.p, faceF.p, vertStart.p, vertFlags.p, P.p, (uint32_t)nf, (uint32_t)nv}; }
};

unsigned grid(uint64_t n) { return (unsigned)((n + DR_SD_BLOCK - 1) / DR_SD_BLOCK); }

}  // namespace

extern "C" int dr_loop_subdivide_device(const uint32_t* indices, uint64_t nfaces, const float* P, uint64_t nverts, int32_t nlevels,
                                        float* P_out, float* N_out, uint32_t* indices_out, uint64_t vert_cap, uint64_t face_cap,
                                        uint64_t* nverts_out, uint64_t* nfaces_out) {
  SdLevel0 l0;
  int rc = sd_prepare("dr_loop_subdivide_device", indices, nfaces, P, nverts, nlevels, l0);
  if (rc != DR_OK) return rc;
  bool done = false;
  rc = sd_check_outputs("dr_loop_subdivide_device", l0, P_out, N_out, indices_out, vert_cap, face_cap, nverts_out, nfaces_out, &done);
  if (rc != DR_OK || done) return rc;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return dr_fail(DR_ERR_NO_DEVICE, "dr_loop_subdivide_device before dr_init");
  const bool dbg = dr_opt("DARTRAY_VERBOSE").toInt(0) >= 2;
  hipStream_t s = 0;
  const int L = nlevels;
  const uint64_t nfL = l0.nf[L], nvL = l0.nv[L];

  // Level l lives in set (L - l) & 1: the last level in set 0, sized for it; set 1 never holds more than level L - 1.
  Level set[2];
  ST(set[0].alloc(nfL, nvL));
  ST(set[1].alloc(L >= 1 ? l0.nf[L - 1] : 1, L >= 1 ? l0.nv[L - 1] : 1));
  Buf<int32_t> edgeVert;
  Buf<uint32_t> created, blk, trigOff;
  Buf<double> trigW;
  Buf<float> Plimit, N;
  const uint64_t maxSlots = L >= 1 ? 3 * l0.nf[L - 1] : 0, maxEdges = L >= 1 ? l0.ne[L - 1] : 0;
  ST(edgeVert.alloc(maxSlots));
  ST(created.alloc(maxEdges));
  ST(blk.alloc((maxSlots + DR_SD_BLOCK - 1) / DR_SD_BLOCK + 1));
  const size_t nOff = l0.trigInterior.size();
  ST(trigOff.alloc(2 * nOff));
  ST(trigW.alloc(l0.trigW.size()));
  ST(Plimit.alloc(3 * nvL));
  ST(N.alloc(3 * nvL));
  Event e0, e1;
  ST(hipEventCreate(&e0.e));
  ST(hipEventCreate(&e1.e));

  Level& first = set[L & 1];
  ST(hipMemcpyAsync(first.faceV.p, l0.faceV.data(), l0.faceV.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(first.faceF.p, l0.faceF.data(), l0.faceF.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(first.vertStart.p, l0.vertStart.data(), l0.vertStart.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(first.vertFlags.p, l0.vertFlags.data(), l0.vertFlags.size(), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(first.P.p, P, 3 * nverts * sizeof(float), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(trigOff.p, l0.trigInterior.data(), nOff * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  ST(hipMemcpyAsync(trigOff.p + nOff, l0.trigBoundary.data(), nOff * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  if (!l0.trigW.empty()) ST(hipMemcpyAsync(trigW.p, l0.trigW.data(), l0.trigW.size() * sizeof(double), hipMemcpyHostToDevice, s));

  ST(hipEventRecord(e0.e, s));
  for (int l = 0; l < L; ++l) {
    const Level& cur = set[(L - l) & 1];
    const Level& nxt = set[(L - l - 1) & 1];
    const SdMesh m = cur.mesh(l0.nf[l], l0.nv[l]);
    const uint32_t nslots = 3u * m.nf, ncreated = (uint32_t)l0.ne[l], nblk = grid(nslots);
    hipLaunchKernelGGL(k_subdiv_even, dim3(grid(m.nv)), dim3(DR_SD_BLOCK), 0, s, m, nxt.P.p, nxt.vertFlags.p);
    hipLaunchKernelGGL(k_subdiv_edge_count, dim3(nblk), dim3(DR_SD_BLOCK), 0, s, m, nslots, blk.p);
    hipLaunchKernelGGL(k_subdiv_scan, dim3(1), dim3(1024), 0, s, blk.p, nblk);
    hipLaunchKernelGGL(k_subdiv_edge_scatter, dim3(nblk), dim3(DR_SD_BLOCK), 0, s, m, nslots, blk.p, ncreated, edgeVert.p, created.p);
    hipLaunchKernelGGL(k_subdiv_odd, dim3(grid(ncreated)), dim3(DR_SD_BLOCK), 0, s, m, created.p, ncreated, nxt.P.p, nxt.vertFlags.p,
                       nxt.vertStart.p);
    hipLaunchKernelGGL(k_subdiv_topology, dim3(grid(m.nf)), dim3(DR_SD_BLOCK), 0, s, m, edgeVert.p, nxt.faceV.p, nxt.faceF.p, nxt.vertStart.p);
    ST(hipGetLastError());
  }
  SdMesh m = set[0].mesh(nfL, nvL);
  hipLaunchKernelGGL(k_subdiv_limit, dim3(grid(nvL)), dim3(DR_SD_BLOCK), 0, s, m, Plimit.p);
  m.P = Plimit.p;
  const SdTrig trig{trigOff.p, trigOff.p + nOff, trigW.p};
  hipLaunchKernelGGL(k_subdiv_normals, dim3(grid(nvL)), dim3(DR_SD_BLOCK), 0, s, m, trig, N.p);
  ST(hipGetLastError());
  ST(hipEventRecord(e1.e, s));

  ST(hipMemcpyAsync(P_out, Plimit.p, 3 * nvL * sizeof(float), hipMemcpyDeviceToHost, s));
  ST(hipMemcpyAsync(N_out, N.p, 3 * nvL * sizeof(float), hipMemcpyDeviceToHost, s));
  ST(hipMemcpyAsync(indices_out, set[0].faceV.p, 3 * nfL * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  ST(hipStreamSynchronize(s));
  if (dbg) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0.e, e1.e);
    fprintf(stderr, "[dartray_hip] dr_loop_subdivide_device: %llu -> %llu faces, %llu vertices, %d levels: %.3f ms on the device (HIP events: the levels, limit and normals; uploads and copy-out excluded)\n",
            (unsigned long long)nfaces, (unsigned long long)nfL, (unsigned long long)nvL, L, ms);
  }
  return DR_OK;
}
