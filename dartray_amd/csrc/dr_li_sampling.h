// dr_li_sampling.h -- what the units outside dr_kernels.hip share of sampling inside Li: the sample's keyed in-Li stream, the scrambled
// radical inverses with Sample02, and UniformSampleSphere.  One definition each:
//   li_stream           moved here from dr_shade_whitted.hip (k_shade_whitted, k_shade_ao);
//   scrambled_radical   moved here from dr_sampler_strat.hip, where it was export_radical (k_export_samples, k_shade_ao): VanDerCorput and
//                       Sobol2 themselves live in dr_kernels.hip, which changes only with new profiling passes (see dr_shade_common.h);
//   W_SCR0 / W_SCR1, new_scramble, load_scramble   the scramble words of the fold / emit integrators, which k_shade_ao, k_shade_prt and
//                       k_shade_gprt each spelt out;
//   UniformSampleSphere the lines sphere_sample (dr_device.h, which the same profiles pin) has inline, as a function of their own:
//                       tests/test_ao_integrator.py holds the two together, line for line.
// Included INSIDE the unit's layout namespace (DR_NS), behind dr_kernels.h and dr_rng.h: includes nothing itself.
#ifndef DR_LI_SAMPLING_H
#define DR_LI_SAMPLING_H

// The sample's keyed in-Li stream (kind 2 of (pixel, sample): DESIGN.md 2.7) at its first draw.  In every sampler mode: the host-buffer
// mode's recorded tail is not read (a ray tree's draws have no useful bound), its pixels and seed key the stream.
DR_DEV DartRandom li_stream(const RenderParams& rp, const BatchState& st, uint32_t slot) {
  const int2 xy = st.pix[slot >> rp.sppShift];
  const uint64_t pixelIndex = (uint64_t)(xy.y - rp.extY0) * (uint64_t)rp.extW + (uint64_t)(xy.x - rp.extX0);
  DartRandom rng;
  rng.seed(dr_counter_key(rp.seed, pixelIndex, (uint64_t)(slot & (uint32_t)(rp.spp - 1)), 2));
  return rng;
}

// VanDerCorput (sobol false) / Sobol2 (sobol true) of index n under a scramble word (montecarlo.dart:486-504): a 24-bit integer times
// 2^-24, exact in f32 and never above ONE_MINUS_EPSILON
DR_DEV float scrambled_radical(uint32_t n, uint32_t scramble, bool sobol) {
  if (!sobol) return (float)((__brev(n) ^ scramble) >> 8) * 5.9604644775390625e-8f;
  for (uint32_t v = 1u << 31; n != 0; n >>= 1, v ^= v >> 1)
    if (n & 1u) scramble ^= v;
  return (float)(scramble >> 8) * 5.9604644775390625e-8f;
}
DR_DEV void Sample02(uint32_t n, const uint32_t scramble[2], double sample[2]) {  // montecarlo.dart:507-511
  sample[0] = scrambled_radical(n, scramble[0], false);
  sample[1] = scrambled_radical(n, scramble[1], true);
}

// The scramble of a fold / emit integrator (k_shade_ao, k_shade_prt, k_shade_gprt): `scramble = [rng.randomUint(), rng.randomUint()]` at the
// camera hit -- draws 0 and 1 of the sample's in-Li stream -- kept in two slot words no other kernel of such a render touches (no MIS ray)
// and reloaded by the later stages.
enum { W_SCR0 = F_MISD, W_SCR1 = F_MISD + 1 };
DR_DEV void new_scramble(const RenderParams& rp, const BatchState& st, uint32_t slot, const SlotRef& sr, uint32_t scramble[2]) {
  DartRandom rng = li_stream(rp, st, slot);
  scramble[0] = rng.randomUint();
  scramble[1] = rng.randomUint();
  sr.u32<W_SCR0>() = scramble[0];
  sr.u32<W_SCR1>() = scramble[1];
}
DR_DEV void load_scramble(const SlotRef& sr, uint32_t scramble[2]) {
  scramble[0] = sr.u32<W_SCR0>();
  scramble[1] = sr.u32<W_SCR1>();
}

DR_DEV F3 UniformSampleSphere(double u1, double u2) {  // montecarlo.dart:113-120
  const double z = 1.0 - 2.0 * u1;
  const double r = sqrt(fmax(0.0, 1.0 - z * z));
  const double phi = 2.0 * DR_PI * u2;
  return f3(r * cos(phi), r * sin(phi), z);
}

#endif
