// dr_sampler_adaptive.hip -- the decision of the adaptive sampler (DR_SAMPLER_ADAPTIVE):
//   k_adaptive_decide   AdaptiveSampler.needsSupersampling, method "contrast" (samplers/adaptive_sampler.dart:170-183), for every
//                       pixel of a first-pass batch, between the batch's last stage and its film step
//
// Both passes of the sampler are the LD pipeline (dr_kernels.hip) unchanged.  This kernel reads the radiances k_film is about to
// add, decides per pixel, appends the pixels that need maxSamples to the render's device list and RETIRES them from the batch's
// film step: their entry of the batch's pixel array moves far outside every film window, where k_film's own clamps add nothing --
// neither to the pixel itself nor to its neighbours under a wide filter (reportResults returns false: the reference never calls
// addSample for these samples, adaptive_sampler.dart:144-147).  Compiled once per state layout (the slot accessors), with
// -ffp-contract=off.
#include "dr_kernels.h"
#include "dr_wave.h"

#ifdef DR_NS
namespace DR_NS {
#endif

#define DR_ADAPT_CHUNK 1024          // samples of one workgroup per pass, as k_film's
#define DR_ADAPT_RETIRED (-(1 << 28))  // raster x and y of a retired pixel: |imageX| + any filter width stays an exact int

// Luminance of the sample k_film would add for slot s: L (+ the deferred last light term of a path that ended), then the
// guards of sampler_renderer.dart:181-193, then Spectrum.luminance of what is left -- in f64, like clum everywhere.
DR_DEV double adaptive_lum(const RenderParams& rp, const BatchState& st, uint32_t s) {
  const SlotRef sr = SlotRef::of(st, s);
  C3 L = ldcf<F_L>(sr);
  if (rp.deferredNee) {
    const uint32_t flags = sr.u32<F_FLAGS>();
    const int occ = sr.i32<F_SHOCC>();
    const C3 Ld1 = ldcf<F_LD1>(sr);
    if ((flags & PF_DEFERRED) && occ == 0) L = cadd(L, Ld1);
  }
  const double lum = clum(L);
  if (L.r != L.r || L.g != L.g || L.b != L.b) L = C3{0.f, 0.f, 0.f};
  else if (lum < -1e-5) L = C3{0.f, 0.f, 0.f};
  else if (isinf(lum)) L = C3{0.f, 0.f, 0.f};
  return clum(L);
}

// The workgroup geometry is k_film's: below 64 spp a workgroup owns 1024 consecutive slots = 1024 / spp whole pixels and one pass;
// from 64 spp on it owns 16 pixels and walks their samples 64 at a time.  Lane = sample parks the luminance in LDS (row pitch
// seg + 1 doubles: the lanes of the adding loop start in different banks), lane = pixel continues the pixel's serial f64 sum
// (((0 + lum_0) + lum_1) + ...) across the passes.  The test |lum_i - Lavg| / Lavg > 0.5 is independent per sample: lane = sample
// again (one pass: from LDS; several: the slot is read a second time), any hit raises the pixel's flag.  Lavg == 0 divides to NaN
// or +-inf - inf: a black pixel is never flagged (the expression is the reference's, literally).
// pix is the batch's own part of the render's pixel array (st.pix): nothing reads a first-pass batch's entries after its film step.
// counts[0]: flagged pixels so far (the list's length), counts[1]: those inside the film window (DrRenderStats.film_samples).
__global__ void __launch_bounds__(256) k_adaptive_decide(RenderParams rp, BatchState st, uint32_t npix, int2* pix, int2* list, uint32_t* counts,
                                                         uint32_t listCap) {
  __shared__ double s_lum[DR_ADAPT_CHUNK + DR_ADAPT_CHUNK / 2];
  __shared__ double s_sum[DR_ADAPT_CHUNK / 2];
  __shared__ uint32_t s_flag[DR_ADAPT_CHUNK / 2];
  const uint32_t spp = (uint32_t)rp.spp;
  const bool tiled = spp >= 64u;
  const uint32_t seg = tiled ? 64u : spp;
  const uint32_t segShift = tiled ? 6u : (uint32_t)rp.sppShift;
  const uint32_t str = seg + 1u;
  const uint32_t nPixBlk = DR_ADAPT_CHUNK >> segShift;  // 16 (tiled) ... 512 (2 spp)
  const uint32_t p0 = blockIdx.x * nPixBlk;
  const uint32_t nPass = tiled ? spp >> 6 : 1u;
  for (uint32_t pass = 0; pass < nPass; ++pass) {
    if (pass) __syncthreads();  // the previous pass's rows have been summed
    for (uint32_t e = threadIdx.x; e < DR_ADAPT_CHUNK; e += 256u) {
      const uint32_t pl = e >> segShift, j = e & (seg - 1u);
      const uint64_t s64 = (uint64_t)(p0 + pl) * spp + (uint64_t)pass * seg + j;
      double lum = 0.0;
      if (p0 + pl < npix && s64 < st.nslots) lum = adaptive_lum(rp, st, (uint32_t)s64);
      s_lum[pl * str + j] = lum;
    }
    __syncthreads();
    for (uint32_t pl = threadIdx.x; pl < nPixBlk; pl += 256u) {
      double a = pass ? s_sum[pl] : 0.0;
      for (uint32_t i = 0; i < seg; ++i) a = a + s_lum[pl * str + i];
      s_sum[pl] = a;
    }
  }
  __syncthreads();
  for (uint32_t pl = threadIdx.x; pl < nPixBlk; pl += 256u) {
    s_sum[pl] = s_sum[pl] / (double)spp;  // Lavg /= count
    s_flag[pl] = 0u;
  }
  __syncthreads();
  for (uint32_t pass = 0; pass < nPass; ++pass)
    for (uint32_t e = threadIdx.x; e < DR_ADAPT_CHUNK; e += 256u) {
      const uint32_t pl = e >> segShift, j = e & (seg - 1u);
      const uint64_t s64 = (uint64_t)(p0 + pl) * spp + (uint64_t)pass * seg + j;
      if (p0 + pl < npix && s64 < st.nslots) {
        const double lum = nPass == 1u ? s_lum[pl * str + j] : adaptive_lum(rp, st, (uint32_t)s64);
        const double Lavg = s_sum[pl];
        if (fabs(lum - Lavg) / Lavg > 0.5) s_flag[pl] = 1u;  // (every writer stores the same word)
      }
    }
  __syncthreads();
  // one reservation per wave and trip (the whole wave reaches it: the trip count depends on the workgroup only)
  for (uint32_t base = 0; base < nPixBlk; base += 256u) {
    const uint32_t pl = base + threadIdx.x, p = p0 + pl;
    const bool flagged = pl < nPixBlk && p < npix && s_flag[pl] != 0u;
    int2 xy = make_int2(0, 0);
    if (flagged) xy = pix[p];
    const bool inFilm = flagged && xy.x >= rp.left && xy.x < rp.left + rp.width && xy.y >= rp.top && xy.y < rp.top + rp.height;
    const unsigned long long m = __ballot(flagged), mIn = __ballot(inFilm);
    if (m == 0ull) continue;
    const int lane = lane_id(), leader = __ffsll((long long)m) - 1;
    uint32_t at = 0u;
    if (lane == leader) {
      at = atomicAdd(counts, (uint32_t)__popcll(m));
      if (mIn) atomicAdd(counts + 1, (uint32_t)__popcll(mIn));
    }
    at = (uint32_t)__shfl((int)at, leader) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (flagged) {
      if (at < listCap) list[at] = xy;
      pix[p] = make_int2(DR_ADAPT_RETIRED, DR_ADAPT_RETIRED);
    }
  }
}

void launch_adaptive_decide(const RenderParams& rp, const BatchState& st, uint32_t npix, int2* pix, int2* list, uint32_t* counts,
                            uint32_t listCap, hipStream_t s) {
  const uint32_t pixBlk = rp.spp >= 64 ? 16u : (uint32_t)(DR_ADAPT_CHUNK / rp.spp);
  const uint32_t nblk = (npix + pixBlk - 1u) / pixBlk;
  if (nblk == 0) return;
  hipLaunchKernelGGL(k_adaptive_decide, dim3(nblk), dim3(256), 0, s, rp, st, npix, pix, list, counts, listCap);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
