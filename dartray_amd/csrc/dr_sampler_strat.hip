// dr_sampler_strat.hip -- the on-device stratified sampler (DR_SAMPLER_STRATIFIED / _NOJITTER) and the sample dump of
// dr_generate_samples:
//   k_gen_strat_pixel / k_gen_strat_lhs  StratifiedSampler.getMoreSamples (samplers/stratified_sampler.dart:67-124;
//                                        StratifiedSample1D/2D, Shuffle, LatinHypercube: core/montecarlo.dart:270-325)
//   k_export_samples                     a batch's sample vectors, either form -> [slot][stride] floats
//
// The sampler writes the float sample form (BatchState, dr_kernels.h): k_raygen, the shade kernels and k_film read it as they
// read a host buffer's vectors.  Compiled once per state layout like dr_kernels.hip (the sample region starts behind the
// layout's state words), with -ffp-contract=off.
#include "dr_sampler_lhs.h"

#ifdef DR_NS
namespace DR_NS {
#endif

#include "dr_li_sampling.h"

// ---------------------------------------------------------------------------
// Stratified sampler (samplers/stratified_sampler.dart:67-124), DR_SAMPLER_STRATIFIED(_NOJITTER): float sample form.
// Streams: kind 3 of (pixel, 0) -- the pixel's strata and shuffles, k_gen_strat_pixel; kind 4 of
// (pixel, sample) -- the LatinHypercube draws of the integrator's slots, k_gen_strat_lhs.
// ---------------------------------------------------------------------------
// r % m for the wave-uniform divisor m: mulhi(r, floor(2^32 / m)) is r / m or one less (s_magic as in k_gen_samples)
DR_DEV int magic_rem(uint32_t r, uint32_t m, const uint32_t* s_magic) {
  uint32_t rem = r - __umulhi(r, s_magic[m]) * m;
  if (rem >= m) rem -= m;
  return (int)rem;
}

// lane = pixel.  Fields 0..4 of the pixel's spp sample vectors in a lane-major LDS table, entry (field f, sample i) of lane l
// at dword (f * spp + i) * LN + l: the generation and the two Fisher-Yates shuffles (random rows) keep every lane in its own
// bank.  LN = blockDim.x <= 64 lanes, as many as fit 80 KB of tables (launch_gen_samples).  Write-out: from 64 spp on a
// lane's 64 consecutive entries of a field are one tile's whole 256-byte run and it stores them itself, 16 bytes at a
// time; below, the workgroup's slots are contiguous and consecutive lanes store consecutive slots.
__global__ void __launch_bounds__(64) k_gen_strat_pixel(RenderParams rp, BatchState st, uint32_t npix, int xs) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  const int LN = (int)blockDim.x, lane = (int)threadIdx.x, spp = rp.spp;
  float* tab = (float*)s_raw;                                  // [5 * spp][LN]
  uint32_t* s_magic = (uint32_t*)s_raw + (size_t)5 * spp * LN;  // [spp + 1]: floor(2^32 / m)
  const uint32_t p0 = blockIdx.x * (uint32_t)LN, p = p0 + (uint32_t)lane;
  for (int m = 1 + lane; m <= spp; m += LN) s_magic[m] = m == 1 ? 0xffffffffu : (uint32_t)(0x100000000ull / (uint32_t)m);
  __syncthreads();
  const bool live = p < npix;
  auto at = [&](int f, int i) -> float& { return tab[((size_t)f * spp + i) * LN + lane]; };
  if (live) {
    const int2 xy = st.pix[p];
    const uint64_t pixelIndex = (uint64_t)(xy.y - rp.extY0) * (uint64_t)rp.extW + (uint64_t)(xy.x - rp.extX0);
    DartRandom rng;
    rng.seed(dr_counter_key(rp.seed, pixelIndex, 0ull, 3));
    const bool jitter = rp.samplerMode == DR_SAMPLER_STRATIFIED;
    const int ys = rp.spp / xs;
    const double dx = 1.0 / (double)xs, dy = 1.0 / (double)ys;
    // the image sample is shifted to the pixel INSIDE the Float32List (stratified_sampler.dart:97-100): imageX is
    // f32(f32(u) + px).  The vector holds the fraction f32(f32(u) + px) - px (exact), so that (double)px + it is that imageX.
    const float fpx = (float)xy.x, fpy = (float)xy.y;
    for (int pass = 0; pass < 2; ++pass)  // StratifiedSample2D (montecarlo.dart:279-292): image, then lens
      for (int y = 0, i = 0; y < ys; ++y)
        for (int x = 0; x < xs; ++x, ++i) {
          const double jx = jitter ? rng.randomFloat() : 0.5;
          const double jy = jitter ? rng.randomFloat() : 0.5;
          float u = lhs_value(x, jx, dx), v = lhs_value(y, jy, dy);
          if (pass == 0) {
            u = (u + fpx) - fpx;
            v = (v + fpy) - fpy;
          }
          at(2 * pass, i) = u;
          at(2 * pass + 1, i) = v;
        }
    const double invTot = 1.0 / (double)spp;  // StratifiedSample1D (montecarlo.dart:270-277): time
    for (int i = 0; i < spp; ++i) at(4, i) = lhs_value(i, jitter ? rng.randomFloat() : 0.5, invTot);
    for (int i = 0; i < spp; ++i) {  // Shuffle(lensSamples, 0, spp, 2) (montecarlo.dart:294-303)
      const int other = i + magic_rem(rng.randomUint(), (uint32_t)(spp - i), s_magic);
      const float a = at(2, i), b = at(3, i);
      at(2, i) = at(2, other);
      at(3, i) = at(3, other);
      at(2, other) = a;
      at(3, other) = b;
    }
    for (int i = 0; i < spp; ++i) {  // Shuffle(timeSamples, 0, spp, 1)
      const int other = i + magic_rem(rng.randomUint(), (uint32_t)(spp - i), s_magic);
      const float a = at(4, i);
      at(4, i) = at(4, other);
      at(4, other) = a;
    }
  }
  if (spp >= 64) {
    if (!live) return;
    const uint32_t* cols = (const uint32_t*)s_raw + lane;  // entry e of this lane's column is cols[e * LN]
    const size_t tile0 = ((size_t)p * (size_t)spp) >> 6;
    for (int f = 0; f < 5; ++f)
      for (int t = 0; t < spp / 64; ++t) {
        uint4* o = (uint4*)(st.sv() + (tile0 + t) * (size_t)st.tileStride + (size_t)f * 64);
        const uint32_t* c = cols + ((size_t)f * spp + (size_t)t * 64) * LN;
        for (int q = 0; q < 16; ++q) o[q] = make_uint4(c[(4 * q + 0) * LN], c[(4 * q + 1) * LN], c[(4 * q + 2) * LN], c[(4 * q + 3) * LN]);
      }
    return;
  }
  __syncthreads();
  const uint32_t nOut = min((uint32_t)LN, npix - p0) * (uint32_t)spp, slot0 = p0 * (uint32_t)spp;
  for (int f = 0; f < 5; ++f)
    for (uint32_t e = lane; e < nOut; e += (uint32_t)LN) {
      const uint32_t pl = e >> rp.sppShift, j = e & (uint32_t)(spp - 1);
      st.sv()[TI64(st.tileStride, slot0 + e) + (size_t)f * 64] = tab[((size_t)f * spp + j) * LN + pl];
    }
}

// lane = sample slot: consecutive lanes are consecutive slots of a tile, so every field's store is one 256-byte run per wave.
// The LatinHypercubes of the integrator's slots: LHS_FILL_SLOTS (dr_sampler_lhs.h).
__global__ void __launch_bounds__(256) k_gen_strat_lhs(RenderParams rp, BatchState st, int nBlocks) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= st.nslots) return;
  const int2 xy = st.pix[slot >> rp.sppShift];
  const uint64_t pixelIndex = (uint64_t)(xy.y - rp.extY0) * (uint64_t)rp.extW + (uint64_t)(xy.x - rp.extX0);
  DartRandom rng;
  rng.seed(dr_counter_key(rp.seed, pixelIndex, (uint64_t)(slot & (uint32_t)(rp.spp - 1)), 4));
  float* sv = st.sv() + TI64(st.tileStride, slot);
  LHS_FILL_SLOTS(rp, sv, rng, nBlocks)
}

// ---------------------------------------------------------------------------
// dr_generate_samples: the sample vectors of a batch as floats, [nslots][stride] in field order.  The float form is copied; the
// compact form (the LD sampler's permuted index per (LD block, slot) + two scramble words per (LD block, pixel)) is evaluated as
// its consumers evaluate it (sv_one / sv_pair in dr_kernels.hip): VanDerCorput for a 1-D value and the x of a pair, Sobol2 for the y.
// ---------------------------------------------------------------------------
// (scrambled_radical: dr_li_sampling.h)
__global__ void __launch_bounds__(256) k_export_samples(RenderParams rp, BatchState st, float* out, int stride) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= st.nslots) return;
  float* o = out + (size_t)slot * stride;
  if (st.svFloat) {
    const float* sv = st.sv() + TI64(st.tileStride, slot);
    for (int f = 0; f < rp.nFloats; ++f) o[f] = sv[(size_t)f * 64];
    return;
  }
  for (int f = 0; f < rp.nFloats; ++f) {
    // LD block of field f and whether f is the second float of a 2-D entry (Appendix B layout: image, lens, time, 1-D slots, 2-D slots)
    const bool twoD = f < 4 || f >= 5 + rp.n1D;
    const int k = f < 5 ? (f >> 1) : (f < 5 + rp.n1D ? f - 2 : 3 + rp.n1D + ((f - 5 - rp.n1D) >> 1));
    const bool second = twoD && (f < 4 ? (f & 1) : ((f - 5 - rp.n1D) & 1));
    const uint8_t* q = st.svIdx() + (size_t)(slot >> 6) * st.tileStride * 4 + (((size_t)k * 64 + (slot & 63u)) << st.idxShift);
    const uint32_t idx = st.idxShift ? (uint32_t)*(const uint16_t*)q : (uint32_t)*q;
    const uint32_t scr = st.svScr[(size_t)(2 * k + (second ? 1 : 0)) * st.pixCap + (slot >> rp.sppShift)];
    o[f] = scrambled_radical(idx, scr, second);
  }
}

// DR_SAMPLER_STRATIFIED(_NOJITTER): the pixel streams, then the per-sample LatinHypercube streams (float form)
void launch_gen_strat(const RenderParams& rp, const BatchState& st, uint32_t npix, int xsamples, hipStream_t s) {
  if (npix == 0) return;
  // lanes (pixels) per workgroup: 20 B per sample and lane of tables, at most 80 KB => two workgroups per CU
  const int ln = rp.spp <= 64 ? 64 : 4096 / rp.spp;
  const size_t lds = (size_t)5 * rp.spp * ln * 4 + ((size_t)rp.spp + 1) * 4;
  static bool attrSet = false;
  if (!attrSet) {
    (void)hipFuncSetAttribute((const void*)k_gen_strat_pixel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attrSet = true;
  }
  hipLaunchKernelGGL(k_gen_strat_pixel, dim3((npix + ln - 1) / ln), dim3(ln), lds, s, rp, st, npix, xsamples);
  hipLaunchKernelGGL(k_gen_strat_lhs, dim3((st.nslots + 255) / 256), dim3(256), 0, s, rp, st, sampler_block_count(rp));
}
void launch_export_samples(const RenderParams& rp, const BatchState& st, float* out, int stride, hipStream_t s) {
  if (st.nslots == 0) return;
  hipLaunchKernelGGL(k_export_samples, dim3((st.nslots + 255) / 256), dim3(256), 0, s, rp, st, out, stride);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
