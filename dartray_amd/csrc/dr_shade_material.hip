// dr_shade_material.hip -- k_shade_material: the first-hit material integrator (DR_INTEGRATOR_MATERIAL), the feature
// integrator's sibling for the two quantities that read a material or a light: one of them as the sample's radiance, so that it reaches the
// film through the same sampler, filter, tiles and shards as a beauty image.
//
//   DR_MATERIAL_CHANNEL_ALBEDO    Kd (matte, plastic) or Kr (mirror, glass) of the hit's material, clamped as getBSDF clamps it; a miss: 0
//   DR_MATERIAL_CHANNEL_EMISSION  isect.Le(-ray.d) at a hit; the sum of the lights' Le(ray) at a miss (the infinite light's map lookup)
//
// Built like k_shade_feature: one lane per slot, slots in order (the camera stage has no list), the channel a template parameter, nothing
// queued.  ALBEDO reads the primitive record and one or two float4 of the material table; EMISSION a hit that is no emitter's costs the
// primitive record alone -- the geometric normal is rebuilt (hit_dg) only where tr.light >= 0 -- and a miss the environment lookup of
// k_shade_probes' miss (escaped_Le).  The values are dr_material_value.h's.  Compiled with -ffp-contract=off, like every unit.
#include "dr_kernels.h"
#include "dr_wave.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_shade_loop.h"
#include "dr_material_value.h"

#define DR_MATERIAL_BLOCK 256

template <int CHANNEL>
__global__ void __launch_bounds__(DR_MATERIAL_BLOCK) k_shade_material(DScene sc, BatchState st, TraceCounters* ctr) {
  __shared__ uint32_t s_hits;
  per_slot_begin(s_hits);
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t hits = 0u;
  for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < st.nslots; slot += stride) {
    const SlotRef sr = SlotRef::of(st, slot);
    const int prim = sr.i32<F_HPRIM>();
    C3 L = C3{0.f, 0.f, 0.f};
    if (prim >= 0) {
      ++hits;
      if (CHANNEL == DR_MATERIAL_CHANNEL_ALBEDO) {
        L = material_albedo(sc, load_tri(sc, (uint32_t)prim).mat);
      } else {
        const HitRec h = hit_rec(sc, (uint32_t)prim);
        if (h.tr.light >= 0) {  // (else isect.Le is 0 whatever the normal)
          const ShadeRec srec = hit_srec(sc, h);
          const F3 o = ld3f<F_RO>(sr), d = ld3f<F_RD>(sr);
          DGeo dg = {};
          hit_dg(sc, h, srec, o, d, sr.f64<F_HT>(), &dg);
          L = material_emission(sc, h.tr, dg.nn, d);
        }
      }
    } else if (CHANNEL == DR_MATERIAL_CHANNEL_EMISSION) {
      L = escaped_Le(sc, sr);
    }
    stcf<F_L>(sr, L);
    sr.u32<F_FLAGS>() = 0u;
  }
  per_slot_end(s_hits, hits, ctr, st.nslots);
}

void launch_shade_material(const DScene& sc, const BatchState& st, const StageQueues& q, int channel, int grid, hipStream_t s) {
  switch (channel) {  // (planRender refused every other value)
    case DR_MATERIAL_CHANNEL_ALBEDO: launch_per_slot<k_shade_material<DR_MATERIAL_CHANNEL_ALBEDO>, DR_MATERIAL_BLOCK>(grid, st.nslots, s, sc, st, q.ctr); break;
    case DR_MATERIAL_CHANNEL_EMISSION: launch_per_slot<k_shade_material<DR_MATERIAL_CHANNEL_EMISSION>, DR_MATERIAL_BLOCK>(grid, st.nslots, s, sc, st, q.ctr); break;
  }
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
