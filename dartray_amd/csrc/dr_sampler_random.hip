// dr_sampler_random.hip -- the on-device random sampler (DR_SAMPLER_RANDOM):
//   k_gen_random  RandomSampler.getMoreSamples, FULL_SAMPLING (samplers/random_sampler.dart:65-85): every value of a sample vector is one
//                 RNG.randomFloat() = Random.nextDouble() (core/rng.dart:36-38); nothing is stratified, shuffled or permuted
//
// The sampler writes the float sample form (BatchState, dr_kernels.h) in the layout k_gen_strat_lhs writes: k_raygen, the shade kernels,
// k_film and k_export_samples read it as they read the stratified sampler's vectors.  Compiled once per state layout like
// dr_sampler_strat.hip (the sample region starts behind the layout's state words), with -ffp-contract=off.
#include "dr_sampler_lhs.h"

#ifdef DR_NS
namespace DR_NS {
#endif

// Stream: kind 6 of (pixel, sample) -- image x, image y, lens u, lens v, time, then the entries of every 1-D slot and
// the pairs of every 2-D slot in request order, which is the field order of the vector (the scene's LdBlock table lists the slots by
// their first field where a slot has several entries, as for LHS_FILL_SLOTS).  Stored: f32(nextDouble) -- exact for the slots, which the
// reference keeps in Float32Lists; the one rounding of this project's sample vector for image fraction, lens and time.
// lane = sample slot: consecutive lanes are consecutive slots of a tile, so every field's store is one 256-byte run per wave, and the
// 2 * nFloats generator steps of a lane are one dependent chain of 32 x 32 -> 64-bit multiply-adds (DartRandom::step, dr_rng.h) that
// the other waves of the CU hide.  No step goes through Random.nextInt here, so DARTRAY_GEN_SLOW_DRAWS has no draw to slow down.
__global__ void __launch_bounds__(256) k_gen_random(RenderParams rp, BatchState st, int nBlocks) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= st.nslots) return;
  const int2 xy = st.pix[slot >> rp.sppShift];
  const uint64_t pixelIndex = (uint64_t)(xy.y - rp.extY0) * (uint64_t)rp.extW + (uint64_t)(xy.x - rp.extX0);
  DartRandom rng;
  rng.seed(dr_counter_key(rp.seed, pixelIndex, (uint64_t)(slot & (uint32_t)(rp.spp - 1)), 6));
  float* sv = st.sv() + TI64(st.tileStride, slot);
  for (int f = 0; f < 5; ++f) sv[(size_t)f * 64] = (float)rng.randomFloat();  // random_sampler.dart:67-71 (time raw: the Lerp is the consumer's)
  for (int k = 3; k < nBlocks; ++k) {                                          // :74-84
    int dst, n;  // the slot's first field and its floats
    if (rp.blocks) {
      const LdBlock lb = rp.blocks[k];
      dst = lb.dst, n = lb.is2D ? 2 * lb.n : lb.n;
    } else if (k < 3 + rp.n1D) {
      dst = 5 + (k - 3), n = 1;
    } else {
      dst = 5 + rp.n1D + 2 * (k - 3 - rp.n1D), n = 2;
    }
    for (int i = 0; i < n; ++i) sv[(size_t)(dst + i) * 64] = (float)rng.randomFloat();
  }
}

// DR_SAMPLER_RANDOM: every vector of the batch in this one launch (a stream's draws are sequential: no block of it can be left for later)
void launch_gen_random(const RenderParams& rp, const BatchState& st, hipStream_t s) {
  if (st.nslots == 0) return;
  hipLaunchKernelGGL(k_gen_random, dim3((st.nslots + 255) / 256), dim3(256), 0, s, rp, st, sampler_block_count(rp));
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
