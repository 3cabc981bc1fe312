// dr_shade_feature.hip -- k_shade_feature: the first-hit feature integrator (DR_INTEGRATOR_FEATURE): one quantity of the camera
// ray's Intersection / DifferentialGeometry (core/intersection.dart, differential_geometry.dart; shapes/triangle.dart, sphere.dart, disk.dart)
// as the sample's radiance, so that it reaches the film through the same sampler, filter, tiles and shards as a beauty image.
//
//   DR_FEATURE_NG     0.5 * (isect.dg.nn + 1)            the geometric normal as Intersection leaves it (reverseOrientation applied)
//   DR_FEATURE_NS     0.5 * (bsdf.dgShading.nn + 1)      Triangle.getShadingGeometry (per-vertex N / S); the geometric one elsewhere
//   DR_FEATURE_DEPTH  t, t, t                            ray.maxDistance after scene.intersect
//   DR_FEATURE_UV     dg.u, dg.v, 0                      mesh uvs, the default uvs (0,0) (1,0) (1,1), the quadrics' parameterisation
//   DR_FEATURE_ID     primitive + 1, material + 1, 1     indices of the scene's arrays; the blue 1 is the coverage mask
// A camera ray that hit nothing stores 0, 0, 0: no light is read.  Every value is >= 0: the renderer's guard blacks out a sample whose
// luminance is below -1e-5.
//
// One lane per slot, slots in order (the camera stage has no list), so a wave's reads of the hit record and the camera ray and its store of
// the radiance are each one run of the tile the state layout was designed around.  The channel is a template parameter: no wave branches on
// it.  Nothing is queued: the render has one stage and traces nothing but the camera rays.  The geometry comes from dr_device.h's own
// helpers, through dr_shade_hit.h's pieces; only (u, v) of a quadric, which quadric_dg does not keep, is restated (feature_quadric_uv,
// dr_feature_value.h: the per-channel values, which k_guides stores too).
// f64 arithmetic, one rounding to the f32 radiance; compiled with -ffp-contract=off, like every unit.
#include "dr_kernels.h"
#include "dr_wave.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_shade_loop.h"
#include "dr_feature_value.h"  // the channels' values: shared with k_guides (dr_guides.hip)

#define DR_FEATURE_BLOCK 256

template <int CHANNEL>
__global__ void __launch_bounds__(DR_FEATURE_BLOCK) k_shade_feature(DScene sc, BatchState st, TraceCounters* ctr) {
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
      const double t = sr.f64<F_HT>();
      if (CHANNEL == DR_FEATURE_DEPTH) {
        L = feature_depth(t);
      } else {
        if (CHANNEL == DR_FEATURE_ID) {
          L = feature_id(prim, load_tri(sc, (uint32_t)prim).mat);
        } else {
          const HitRec h = hit_rec(sc, (uint32_t)prim);
          const ShadeRec srec = hit_srec(sc, h);
          const F3 o = ld3f<F_RO>(sr), d = ld3f<F_RD>(sr);
          DGeo dg = {}, dgs = {};
          // (u, v) of a quadric and the default uvs are not isect.dg's: dr_feature_value.h
          if (!(CHANNEL == DR_FEATURE_UV && feature_uv_without_dg(sc, h, o, d, t, &dg.u, &dg.v))) hit_dg(sc, h, srec, o, d, t, &dg);
          if (CHANNEL == DR_FEATURE_NG) {
            L = feature_normal(dg.nn);
          } else if (CHANNEL == DR_FEATURE_NS) {
            hit_dgs(sc, h, srec, dg, &dgs);  // (a quadric's Shape.getShadingGeometry: a copy)
            L = feature_normal(dgs.nn);
          } else {
            L = feature_uv(dg.u, dg.v);
          }
        }
      }
    }
    stcf<F_L>(sr, L);
    sr.u32<F_FLAGS>() = 0u;
  }
  per_slot_end(s_hits, hits, ctr, st.nslots);
}

void launch_shade_feature(const DScene& sc, const BatchState& st, const StageQueues& q, int channel, int grid, hipStream_t s) {
  switch (channel) {  // (planRender refused every other value)
    case DR_FEATURE_NG: launch_per_slot<k_shade_feature<DR_FEATURE_NG>, DR_FEATURE_BLOCK>(grid, st.nslots, s, sc, st, q.ctr); break;
    case DR_FEATURE_NS: launch_per_slot<k_shade_feature<DR_FEATURE_NS>, DR_FEATURE_BLOCK>(grid, st.nslots, s, sc, st, q.ctr); break;
    case DR_FEATURE_DEPTH: launch_per_slot<k_shade_feature<DR_FEATURE_DEPTH>, DR_FEATURE_BLOCK>(grid, st.nslots, s, sc, st, q.ctr); break;
    case DR_FEATURE_UV: launch_per_slot<k_shade_feature<DR_FEATURE_UV>, DR_FEATURE_BLOCK>(grid, st.nslots, s, sc, st, q.ctr); break;
    case DR_FEATURE_ID: launch_per_slot<k_shade_feature<DR_FEATURE_ID>, DR_FEATURE_BLOCK>(grid, st.nslots, s, sc, st, q.ctr); break;
  }
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
