// dr_sampler_halton.hip -- the on-device Halton sampler (DR_SAMPLER_HALTON):
//   k_halton_count / _scan / _scatter   which indices of a range of the task's sequence fall inside its window
//                                       (HaltonSampler.getMoreSamples' rejection loop, samplers/halton_sampler.dart:63-83)
//   k_gen_halton                        the accepted samples' anchor pixels, key pixels and sample vectors (:69-74, :86-97; RadicalInverse
//                                       and LatinHypercube: core/montecarlo.dart:305-339)
//
// A sample belongs to the image, not to a pixel: slot i of a batch is the i-th ACCEPTED index of the batch's range, in increasing
// order, and carries its own entry of the pixel array (the batch runs at one sample per "pixel").  No atomic decides an order: a
// workgroup counts its accepted lanes (wave ballots), one workgroup scans the counts, and the scatter repeats the test and places every
// index behind the accepted ones before it.  Compiled once per state layout like dr_sampler_strat.hip (k_gen_halton writes the float
// sample form behind the layout's state words), with -ffp-contract=off: every expression below is the reference's f64 expression.
#include "dr_sampler_lhs.h"
#include "dr_wave.h"

#ifdef DR_NS
namespace DR_NS {
#endif

#define DR_HALTON_BLOCK 256  // indices per workgroup of the selection kernels: one entry of the block counts

// The task's window of the sampler extent as HaltonSampler holds it (sampler.dart:40-54: right and bottom are inclusive) and
// delta = max(width, height) (halton_sampler.dart:35,71): the launchers' win[5]
struct HaltonWindow {
  int32_t left, top, right, bottom, delta;
};

// RadicalInverse (montecarlo.dart:327-339), as written: the digit is n % base, the next n is the TRUNCATED PRODUCT n * (1 / base).
template <uint32_t BASE>
DR_DEV double radical_inverse(uint64_t n) {
  double val = 0.0;
  const double invBase = 1.0 / (double)BASE;
  double invBi = invBase;
  while (n > 0) {
    const uint32_t d = (uint32_t)(n % BASE);
    val += (double)d * invBi;
    n = (uint64_t)((double)n * invBase);
    invBi *= invBase;
  }
  return val;
}
DR_DEV double halton_lerp(double t, double v1, double v2) { return v1 * (1.0 - t) + v2 * t; }  // Lerp (common.dart:80-81)
// imageX / imageY of index k (halton_sampler.dart:69-74)
DR_DEV void halton_image(const HaltonWindow& hw, uint64_t k, double* imageX, double* imageY) {
  const double u = radical_inverse<3>(k), v = radical_inverse<2>(k);
  *imageX = halton_lerp(u, (double)hw.left, (double)(hw.left + hw.delta));
  *imageY = halton_lerp(v, (double)hw.top, (double)(hw.top + hw.delta));
}
DR_DEV bool halton_accept(const HaltonWindow& hw, uint64_t k) {  // :78: rejected iff imageX > right || imageY > bottom
  double x, y;
  halton_image(hw, k, &x, &y);
  return !(x > (double)hw.right || y > (double)hw.bottom);
}

// lane = index k0 + i of the range [k0, k0 + n).  blk[b]: accepted lanes of workgroup b.
__global__ void __launch_bounds__(DR_HALTON_BLOCK) k_halton_count(HaltonWindow hw, uint64_t k0, uint32_t n, uint32_t* blk) {
  __shared__ uint32_t s_wave[DR_HALTON_BLOCK / 64];
  const uint32_t i = blockIdx.x * DR_HALTON_BLOCK + threadIdx.x;
  const bool acc = i < n && halton_accept(hw, k0 + i);
  const unsigned long long m = __ballot(acc);
  if (lane_id() == 0) s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0u;
    for (int w = 0; w < DR_HALTON_BLOCK / 64; ++w) sum += s_wave[w];
    blk[blockIdx.x] = sum;
  }
}

// One workgroup: blk[0 .. nblk) becomes its exclusive prefix sum, blk[nblk] the total (the batch's slot count).  A thread owns a
// contiguous run of entries; the runs' sums are scanned inside each wave by shuffles and across the 16 waves through LDS.
__global__ void __launch_bounds__(1024) k_halton_scan(uint32_t* blk, uint32_t nblk) {
  __shared__ uint32_t s_wave[16];
  const uint32_t per = (nblk + 1023u) / 1024u;
  const uint32_t b0 = min(threadIdx.x * per, nblk), b1 = min(b0 + per, nblk);
  uint32_t sum = 0u;
  for (uint32_t b = b0; b < b1; ++b) sum += blk[b];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  uint32_t inc = sum;  // inclusive scan of the wave's 64 sums
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
  if (threadIdx.x == 1023u) blk[nblk] = run;  // (the last thread's run ends at nblk, whatever it owns)
}

// The test again, and every accepted index to its place: the workgroup's offset + the accepted lanes of the waves before this one +
// those of the lower lanes of this wave.  seqIdx has room for n entries (a range of n indices accepts at most n).
__global__ void __launch_bounds__(DR_HALTON_BLOCK) k_halton_scatter(HaltonWindow hw, uint64_t k0, uint32_t n, const uint32_t* blk,
                                                                    unsigned long long* seqIdx) {
  __shared__ uint32_t s_wave[DR_HALTON_BLOCK / 64];
  const uint32_t i = blockIdx.x * DR_HALTON_BLOCK + threadIdx.x;
  const bool acc = i < n && halton_accept(hw, k0 + i);
  const unsigned long long m = __ballot(acc);
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!acc) return;
  uint32_t at = blk[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) at += s_wave[w];
  seqIdx[at] = k0 + i;
}

// lane = slot = accepted sample.  The image sample leaves as its anchor pixel (floor) and the f32 fraction behind it (which may round
// to 1.0f; consumers form (double)px + fraction as for every mode); lens and time are the radical inverses of k + 1 (the reference
// increments currentSample before it draws them, :76-89), time raw.  The integrator's slots: LatinHypercube per 1-D slot, then per
// 2-D slot, on the stream kind 5 of (k, 0) -- LHS_FILL_SLOTS (dr_sampler_lhs.h), the loop k_gen_strat_lhs runs as well.
// The draws inside Li come from the stream kind 2 of (k, 0).  The shade kernels key that stream by the slot's pixel -- its index in the
// full sampler extent, (y - extY0) * extW + (x - extX0), and the sample number, 0 at one sample per pixel entry (TailSrc, dr_kernels.hip) --
// so the slot gets a second, KEY pixel whose index is k; the shade stages of a Halton batch read that array as their pixel array (nothing
// else of a shade kernel looks at a pixel), k_raygen and k_film the anchors.  Samples anchored in one pixel thus draw from different
// streams.  (planRender keeps k / extW inside an int.)
__global__ void __launch_bounds__(256) k_gen_halton(RenderParams rp, BatchState st, HaltonWindow hw, const unsigned long long* seqIdx, int2* pix,
                                                    int2* keyPix, int nBlocks) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= st.nslots) return;
  const uint64_t k = seqIdx[slot];
  double imageX, imageY;
  halton_image(hw, k, &imageX, &imageY);
  const double fx = floor(imageX), fy = floor(imageY);
  pix[slot] = make_int2((int)fx, (int)fy);
  keyPix[slot] = make_int2(rp.extX0 + (int)(k % (uint64_t)rp.extW), rp.extY0 + (int)(k / (uint64_t)rp.extW));
  float* sv = st.sv() + TI64(st.tileStride, slot);
  sv[0 * 64] = (float)(imageX - fx);
  sv[1 * 64] = (float)(imageY - fy);
  sv[2 * 64] = (float)radical_inverse<5>(k + 1);
  sv[3 * 64] = (float)radical_inverse<7>(k + 1);
  sv[4 * 64] = (float)radical_inverse<11>(k + 1);
  DartRandom rng;
  rng.seed(dr_counter_key(rp.seed, k, 0ull, 5));
  LHS_FILL_SLOTS(rp, sv, rng, nBlocks)
}

// The accepted indices of [k0, k0 + n), in order, to seqIdx; their number to blk[(n + 255) / 256] (blk: that many entries + 1).
void launch_halton_select(const int32_t win[5], uint64_t k0, uint32_t n, uint32_t* blk, unsigned long long* seqIdx, hipStream_t s) {
  if (n == 0) return;
  const HaltonWindow hw = {win[0], win[1], win[2], win[3], win[4]};
  const uint32_t nblk = (n + DR_HALTON_BLOCK - 1u) / DR_HALTON_BLOCK;
  hipLaunchKernelGGL(k_halton_count, dim3(nblk), dim3(DR_HALTON_BLOCK), 0, s, hw, k0, n, blk);
  hipLaunchKernelGGL(k_halton_scan, dim3(1), dim3(1024), 0, s, blk, nblk);
  hipLaunchKernelGGL(k_halton_scatter, dim3(nblk), dim3(DR_HALTON_BLOCK), 0, s, hw, k0, n, blk, seqIdx);
}
// st.nslots accepted samples (seqIdx): pix[slot], keyPix[slot] and the float-form sample vectors
void launch_gen_halton(const RenderParams& rp, const BatchState& st, const int32_t win[5], const unsigned long long* seqIdx, int2* pix, int2* keyPix,
                       hipStream_t s) {
  if (st.nslots == 0) return;
  const HaltonWindow hw = {win[0], win[1], win[2], win[3], win[4]};
  hipLaunchKernelGGL(k_gen_halton, dim3((st.nslots + 255) / 256), dim3(256), 0, s, rp, st, hw, seqIdx, pix, keyPix, sampler_block_count(rp));
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
