// dr_sampler_lhs.h -- what the stratified and the Halton device sampler share (dr_sampler_strat.hip, dr_sampler_halton.hip):
// how many LD blocks a sample vector has (also dr_sampler_random.hip's), and the LatinHypercube of the integrator's slots (core/montecarlo.dart:305-325).
#ifndef DR_SAMPLER_LHS_H
#define DR_SAMPLER_LHS_H

#include "dr_kernels.h"
#include "dr_rng.h"

// LD blocks of one sample vector: image, lens, time, one per slot -- rp.blocks' where slots have several entries, else counted from the fields
__host__ __device__ inline int sampler_block_count(const RenderParams& rp) {
  return rp.blocks ? rp.nBlocks : 3 + rp.n1D + (rp.nFloats - 5 - rp.n1D) / 2;
}

// min((i + u) * delta, ONE_MINUS_EPSILON) in f64, stored to a Float32List (montecarlo.dart:275,288-289,311-312)
DR_DEV float lhs_value(int i, double u, double delta) {
  return (float)fmin(((double)i + u) * delta, 0.9999999403953552);
}

// LatinHypercube (montecarlo.dart:305-325) per 1-D, then per 2-D slot of one slot's float-form vector (field f at sv[f * 64]): n * dims randomFloat, then dims * n randomUint (also for n == 1).
// A macro, not a function: expanded in place the two kernels compile to the very code they had with their own copies of the loop (as a function
// hipcc orders a few instructions differently), which is what lets their speed go unmeasured.
#define LHS_FILL_SLOTS(rp, sv, rng, nBlocks)                                                                                  \
  for (int k = 3; k < (nBlocks); ++k) {                                                                                       \
    int dst, n, dims; /* the block's first field, its entries and their dimension */                                          \
    if ((rp).blocks) {                                                                                                        \
      const LdBlock lb = (rp).blocks[k];                                                                                      \
      dst = lb.dst, n = lb.n, dims = lb.is2D ? 2 : 1;                                                                         \
    } else if (k < 3 + (rp).n1D) {                                                                                            \
      dst = 5 + (k - 3), n = 1, dims = 1;                                                                                     \
    } else {                                                                                                                  \
      dst = 5 + (rp).n1D + 2 * (k - 3 - (rp).n1D), n = 1, dims = 2;                                                           \
    }                                                                                                                         \
    const double delta = 1.0 / (double)n;                                                                                     \
    for (int i = 0; i < n; ++i)                                                                                               \
      for (int d = 0; d < dims; ++d) (sv)[(size_t)(dst + dims * i + d) * 64] = lhs_value(i, (rng).randomFloat(), delta);      \
    for (int d = 0; d < dims; ++d)                                                                                            \
      for (int j = 0; j < n; ++j) {                                                                                           \
        const int other = j + (int)((rng).randomUint() % (uint32_t)(n - j));                                                  \
        if (other != j) {                                                                                                     \
          float* a = (sv) + (size_t)(dst + dims * j + d) * 64;                                                                \
          float* b = (sv) + (size_t)(dst + dims * other + d) * 64;                                                            \
          const float t = *a;                                                                                                 \
          *a = *b;                                                                                                            \
          *b = t;                                                                                                             \
        }                                                                                                                     \
      }                                                                                                                       \
  }

#endif
