// dr_shade_ao.hip -- k_shade_ao: AmbientOcclusionIntegrator.Li (surface_integrators/ambient_occlusion_integrator.dart:28-53), one
// occlusion ray per slot and stage.
//
// A camera hit sends nSamples rays Ray(p, w_i, minDist, maxDist), w_i = UniformSampleSphere(Sample02(i, scramble)) flipped into the
// hemisphere of n = FaceForward(isect.dg.nn, -ray.direction), and returns Spectrum(nClear / nSamples), nClear the rays for which
// !scene.intersectP.  The kernel only produces and consumes rays; every ray is traced by the any-hit traversal launch the batch runner
// puts between two stages (dr_batch.hip), so the scene's traversal kernel choice and its switches apply unchanged.  A stage
//   emit == 0    sets up the camera hit: p = bsdf.dgShading.p, n, the two rng.randomUint() of the scramble, nClear = 0; an escaped
//                camera ray stores the lights' Le(ray) (sampler_renderer.dart:87-92) and leaves the lists;
//   fold >= 0    folds ray `fold` in: ++nClear unless the traversal found an occluder;
//   emit >= 0    queues ray `emit`;
//   fold == nSamples - 1 (the last ray)   stores L = Spectrum(nClear / nSamples).
// The host (BatchRunner::stage) names both indices: within a round of the stage loop stage b folds ray b - 1 in and queues ray b; the
// last stage of a round has no traversal behind it and queues nothing, so the next round's first stage queues without folding.
//
// Draws: the two randomUint() are draws 0 and 1 of the sample's keyed in-Li stream (kind 2), in every sampler mode.
// Per-slot state, in words no other kernel of an AO render touches (no MIS ray, no throughput): W_SCR0, W_SCR1 (dr_li_sampling.h), W_NCLEAR, W_N below.
// F_RO = p, F_RTMIN = minDist and F_SHTMAX = maxDist are written once at the camera hit: every ray of the slot shares them.
//
// Launch geometry is k_shade_whitted's (one 512-thread workgroup per CU for the ~64 KB of queue staging); the kernel needs no light or
// material table; the stage loop, the hit's geometry and the scramble words are the units' shared ones (dr_shade_loop.h, dr_shade_hit.h,
// dr_li_sampling.h).  Compiled with -ffp-contract=off, like every unit.
#include "dr_kernels.h"
#include "dr_rng.h"
#include "dr_wave.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_shade_loop.h"
#include "dr_li_sampling.h"

// per-slot words besides the scramble (dr_li_sampling.h): the clear rays counted so far (i32), n (3 x f32)
enum { W_NCLEAR = F_MISPRIM, W_N = F_BETA };

__global__ void __launch_bounds__(SHADE_BLOCK_OF(true), SHADE_WAVES_OF(true))
    k_shade_ao(DScene sc, RenderParams rp, BatchState st, StageQueues q, int nSamples, int fold, int emit, double minDist, double maxDist) {
  extern __shared__ __align__(16) unsigned char s_dyn[];
  PushStage& s_push = *(PushStage*)s_dyn;
  StageLoop loop = stage_loop_begin(s_push, st, q);
  for (uint32_t it = 0; it < loop.nIter; ++it) {
    uint32_t slot = 0, pf = 0;
    bool again = false, vert = false;  // again: the slot has another stage; vert: a camera hit was set up here (statistics)
    if (stage_loop_slot(loop, q, it, &slot)) {
      const SlotRef sr = SlotRef::of(st, slot);
      bool live = emit != 0;  // (behind the camera hit's stage the lists only hold slots that hit)
      F3 n;
      uint32_t scramble[2];
      int nClear = 0;
      if (emit == 0) {
        const int prim = sr.i32<F_HPRIM>();
        if (prim >= 0) {
          const F3 o = ld3f<F_RO>(sr), d = ld3f<F_RD>(sr);
          DGeo dg, dgs;
          hit_geometry(sc, hit_rec(sc, (uint32_t)prim), o, d, sr.f64<F_HT>(), &dg, &dgs);
          const F3 p = dgs.p;                                           // bsdf.dgShading.p
          n = vdot(dg.nn, vneg(d)) < 0.0 ? vneg(dg.nn) : dg.nn;         // Normal.FaceForward(isect.dg.nn, -ray.direction) (normal.dart:59-61)
          new_scramble(rp, st, slot, sr, scramble);
          st3f<F_RO>(sr, p);  // Ray(p, w, minDist, maxDist): minT is minDist, not the intersection's ray epsilon
          sr.f64<F_RTMIN>() = minDist;
          sr.f64<F_SHTMAX>() = maxDist;
          st3f<W_N>(sr, n);
          live = vert = true;
        } else {
          store_escaped_Le(sc, sr);
        }
      } else {
        nClear = sr.i32<W_NCLEAR>();
        if (emit > 0) {
          n = ld3f<W_N>(sr);
          load_scramble(sr, scramble);
        }
      }
      if (live) {
        if (fold >= 0 && sr.i32<F_SHOCC>() == 0) ++nClear;  // if (!scene.intersectP(r)) ++nClear
        if (emit >= 0) {
          double u[2];
          Sample02((uint32_t)emit, scramble, u);
          F3 w = UniformSampleSphere(u[0], u[1]);
          if (vdot(w, n) < 0.0) w = vneg(w);
          st3f<F_SHD>(sr, w);
          pf = PF_HAS_SH;
        }
        if (fold == nSamples - 1) {
          const float a = (float)((double)nClear / (double)nSamples);  // new Spectrum(nClear / nSamples)
          stcf<F_L>(sr, C3{a, a, a});
        } else {
          sr.i32<W_NCLEAR>() = nClear;
          again = true;
        }
      }
      sr.u32<F_FLAGS>() = pf;
    }
    stage_loop_push(s_push, loop, q, it, false, false, (pf & PF_HAS_SH) != 0, again, slot, Q_MIS_BIT, vert);
  }
  stage_loop_end(s_push, loop, q);
}

void launch_shade_ao(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int nSamples, int fold, int emit,
                     double minDist, double maxDist, int grid, hipStream_t s) {
  launch_shade<k_shade_ao, SHADE_BLOCK_OF(true)>(grid, 0, s, sc, rp, st, q, nSamples, fold, emit, minDist, maxDist);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
