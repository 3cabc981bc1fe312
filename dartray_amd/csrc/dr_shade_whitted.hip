// dr_shade_whitted.hip -- k_shade_whitted: WhittedIntegrator.Li (surface_integrators/whitted_integrator.dart:28-60) for ONE vertex of a
// slot's ray tree, one light per stage.
//
// A vertex is nLights + 1 stages of the stage loop (dr_batch.hip), chained the way k_shade_direct chains its EstimateDirect calls:
//   stage 0              the hit's geometry, L = 0 + isect.Le(wo), light 0 set up;
//   stage s, 0 < s < n   light s - 1 folded in (its shadow ray has been traced in between), light s set up;
//   stage n              light n - 1 folded in; st.L holds the vertex's Le + direct lighting.
// "Set up" is lines 44-58 up to the point where they must trace: sampleLAtPoint with one LightSample.random(rng), bsdf.f(wo, wi) with
// every lobe, the shadow ray and the FINISHED term f * Li * AbsDot(wi, n) * T / pdf (T = 1: no participating media) parked in Ld1; "folded
// in" is `L += Ld1` unless the any-hit traversal found an occluder.  No BSDF-sampling half, no MIS weight, no nsamples.
// Lines 62-69 -- SpecularReflect / SpecularTransmit while ray.depth + 1 < maxDepth -- are k_shade_spec's round (dr_kernels.hip), unchanged:
// it reads what the last stage leaves (L, the hit, ro = p, rtmin = rayEpsilon, ro0) exactly as it reads k_shade_direct's.
//
// Draws: draw number d of the reference's depth-first walk of a sample's ray tree -- every rng.randomFloat() in its
// call order: a vertex's lights in scene order, three each; then the three SpecularReflect burns, the reflected subtree, the three
// SpecularTransmit burns, the transmitted subtree -- is the d-th randomFloat() of the sample's keyed in-Li stream (kind 2).  The slot
// carries the stream's generator state along the walk, so no stage ever re-seeds and skips: the camera vertex seeds it, every stage
// makes its three draws and stores it back, and stage 0 of a deeper vertex first steps it over the Specular* burns made since the
// previous vertex's lights (a handful: counted from a per-slot count and the suspended ancestors' frames).  State and counts live in
// slot words no other kernel of a Whitted render touches (there is no MIS ray): W_LO, W_HI, W_NR, W_CALLS below.
//
// Launch geometry and LDS use are k_shade_direct's general form: one 512-thread workgroup per CU, 2 waves per SIMD, the light and
// material tables in LDS where they fit; the stage loop and the pieces of the hit's geometry are the units' shared ones (dr_shade_loop.h,
// dr_shade_hit.h).  Compiled with -ffp-contract=off, like every unit.
#include <type_traits>

#include "dr_kernels.h"
#include "dr_rng.h"
#include "dr_wave.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_shade_loop.h"
#include "dr_li_sampling.h"  // li_stream

// per-slot words of the draw numbering: the stream's generator state behind the last draw made (u32 lo, hi), the vertices shaded so far
// with ray.depth + 1 < maxDepth, and the Specular* calls that had been made when the previous vertex started (i32)
enum { W_LO = F_MISD, W_HI = F_MISD + 1, W_NR = F_MISPRIM, W_CALLS = F_MISLIGHT };

template <bool LLDS>
__global__ void __launch_bounds__(SHADE_BLOCK_OF(true), SHADE_WAVES_OF(true)) k_shade_whitted(DScene sc, RenderParams rp, BatchState st, StageQueues q, int stage) {
  extern __shared__ __align__(16) unsigned char s_dyn[];
  PushStage& s_push = *(PushStage*)s_dyn;
  using LV = typename std::conditional<LLDS, LdsLights, GlobalLights>::type;
  LV lv;
  if constexpr (LLDS) lv = stage_lights(sc, s_dyn, push_stage_bytes(SHADE_BLOCK_OF(true)));
  else lv = GlobalLights{sc.lights, sc.ltris, sc.lcdf, sc.mats};
  const int nLights = rp.nLights;
  StageLoop loop = stage_loop_begin(s_push, st, q);
  for (uint32_t it = 0; it < loop.nIter; ++it) {
    uint32_t slot = 0, pf = 0;
    bool again = false, vert = false;  // again: the vertex has another stage; vert: a vertex was set up here (statistics)
    if (stage_loop_slot(loop, q, it, &slot)) {
      const SlotRef sr = SlotRef::of(st, slot);
      const uint32_t flags = stage == 0 ? 0u : sr.u32<F_FLAGS>();
      const int prim = sr.i32<F_HPRIM>();
      if (prim >= 0) {
        const HitRec h = hit_rec(sc, (uint32_t)prim);
        const Tri& tr = h.tr;
        const F3 d = ld3f<F_RD>(sr);
        const F3 wo = vneg(d);
        C3 L;
        DartRandom rng;  // the sample's in-Li stream, at this stage's first draw
        DGeo dg, dgs;
        const ShadeRec srec = hit_srec(sc, h);
        const bool fromRay = h.isQuad || h.hasRec;  // later stages and k_shade_spec rebuild such a hit from the ray: F_RO0 keeps its origin
        if (stage == 0) {
          const F3 o = ld3f<F_RO>(sr);
          const double t = sr.f64<F_HT>();
          hit_dg(sc, h, srec, o, d, t, &dg);
          if (fromRay) st3f<F_RO0>(sr, o);
          L = cadd(C3{0.f, 0.f, 0.f}, hit_Le(lv, tr, dg.nn, wo));  // L = Spectrum(0); L += isect.Le(wo)
          st3f<F_RO>(sr, dg.p);
          sr.f64<F_RTMIN>() = ray_epsilon(h.isQuad, t);
          // Where this vertex's draws start in the sample's stream: behind everything the reference has drawn before it calls Li here.
          // The stored state stands behind the previous vertex's last light draw; since then only Specular* calls have drawn, each a
          // BSDFSample.random(rng) -- 3 randomFloat(), 6 generator steps -- whether or not a lobe exists.  Calls made before this vertex
          // starts: of the nR vertices shaded so far with ray.depth + 1 < maxDepth, the sp suspended ancestors are part way -- one call
          // while the reflected child is out (frame state 1), both once the transmitted child is (state 2) -- and the other nR - sp have
          // returned: both calls.  The difference to the count the previous vertex stored is what to step over.
          const int sp = rp.dlSpecular ? st.specSp[slot] : 0;  // (no mirror / glass: one round, every vertex is a camera vertex)
          const int nR = sp == 0 ? 0 : sr.i32<W_NR>();
          int calls = 2 * (nR - sp);
          for (int level = 0; level < sp; ++level)
            calls += (int)(((const SpecFrame*)(st.specFrames + ((size_t)level * st.cap + slot) * DR_SPEC_FRAME_WORDS))->state & 255u);
          if (sp == 0) {
            rng = li_stream(rp, st, slot);  // the camera vertex: draw 0
          } else {
            rng.lo = sr.u32<W_LO>();
            rng.hi = sr.u32<W_HI>();
            for (int i = 6 * (calls - sr.i32<W_CALLS>()); i > 0; --i) rng.step();
          }
          sr.i32<W_NR>() = nR + (sp + 1 < rp.maxDepth ? 1 : 0);
          sr.i32<W_CALLS>() = calls;
          vert = true;
        } else {
          // (a plain triangle's dpdu, dpdv and nn do not depend on the ray)
          hit_dg(sc, h, srec, fromRay ? ld3f<F_RO0>(sr) : F3{0, 0, 0}, d, fromRay ? sr.f64<F_HT>() : 0.0, &dg);
          dg.p = ld3f<F_RO>(sr);
          rng.lo = sr.u32<W_LO>();
          rng.hi = sr.u32<W_HI>();
          L = ldcf<F_L>(sr);
          // light stage - 1: `if (!f.isBlack() && visibility.unoccluded(scene)) L += ...` (whitted_integrator.dart:56-59)
          if ((flags & PF_HAS_SH) && sr.i32<F_SHOCC>() == 0) L = cadd(L, ldcf<F_LD1>(sr));
        }
        if (stage < nLights) {
          hit_dgs(sc, h, srec, dg, &dgs);
          Bsdf bsdf = make_bsdf<true>(lv, dgs, tr.mat);  // isect.getBSDF(ray)
          bsdf.ng = dg.nn;
          const F3 p = bsdf.p, n = bsdf.nn;  // bsdf.dgShading.p / .nn
          // new LightSample.random(rng) (light_sample.dart:46-51): uPos is f32 storage; drawn for delta lights too
          const double u0 = (float)rng.randomFloat();
          const double u1 = (float)rng.randomFloat();
          const double uc = rng.randomFloat();
          sr.u32<W_LO>() = rng.lo;
          sr.u32<W_HI>() = rng.hi;
          const DLight light = lv.light(stage);
          // light.sampleLAtPoint(p, isect.rayEpsilon, ls, ray.time, wi, pdf, visibility)
          F3 wi = F3{0, 0, 0}, shd = F3{0, 0, 0};
          double pdf = 0.0, shTmax = 0.0;
          C3 Li;
          if (light.kind >= DR_LIGHT_POINT) {
            // PointLight (point_light.dart:41-47), SpotLight (spot_light.dart:54-85), DistantLight (distant_light.dart:54-61): pdf = 1
            const F3 lp = F3{light.pos[0], light.pos[1], light.pos[2]};
            const F3 seg = vsub(lp, p);
            pdf = 1.0;
            if (light.kind == DR_LIGHT_DISTANT) {
              wi = lp;
              Li = C3{light.L[0], light.L[1], light.L[2]};
              shd = wi;  // VisibilityTester.setRay(p, eps, wi)
              shTmax = DR_INF;
            } else {
              wi = vnormalize(seg);
              C3 I = C3{light.L[0], light.L[1], light.L[2]};
              if (light.kind == DR_LIGHT_SPOT) {
                const F3 wl = vnormalize(q_vector(light.w2l, vneg(wi)));
                const double costheta = wl.z;
                double fo;
                if (costheta < light.cosTotalWidth) fo = 0.0;
                else if (costheta > light.cosFalloffStart) fo = 1.0;
                else {
                  const double delta = (costheta - light.cosTotalWidth) / (light.cosFalloffStart - light.cosTotalWidth);
                  fo = delta * delta * delta * delta;
                }
                I = cmulD(I, fo);
              }
              Li = cdivD(I, vlen2(seg));
              const double dist = vlen(seg);  // VisibilityTester.setSegment(p, eps, lightPos, 0)
              shd = vdiv(seg, dist);
              shTmax = dist * (1.0 - 0.0);
            }
          } else if (light.kind == DR_LIGHT_INFINITE) {
            // InfiniteAreaLight.sampleLAtPoint (infinite_area_light.dart:92-131); VisibilityTester.setRay
            Li = env_sample_x<false>(sc.env, u0, u1, &wi, &pdf);
            shd = wi;
            shTmax = DR_INF;
          } else {
            // DiffuseAreaLight.sampleLAtPoint (diffuse_area_light.dart:60-70); VisibilityTester.setSegment (visibility_tester.dart:26-29)
            F3 ns;
            const F3 ps = shapeset_sample<true>(sc, lv, light, u0, u1, uc, &ns, p);
            wi = vnormalize(vsub(ps, p));
            pdf = shapeset_pdf<true>(sc, lv, light, p, wi);
            Li = light_L(light, ns, vneg(wi));
            const F3 seg = vsub(ps, p);
            const double dist = vlen(seg);
            shd = vdiv(seg, dist);
            shTmax = dist * (1.0 - 1.0e-3);
          }
          if (!(cblack(Li) || pdf == 0.0)) {
            const C3 f = bsdf_f(bsdf, wo, wi, BSDF_ALL);  // every lobe: the specular ones return nothing from f()
            if (!cblack(f)) {
              st3f<F_SHD>(sr, shd);
              sr.f64<F_SHTMAX>() = shTmax;
              // f * Li * AbsDot(wi, n) * visibility.transmittance(...) / pdf[0], left to right, every product a Spectrum (f32)
              const C3 T = C3{1.f, 1.f, 1.f};
              stcf<F_LD1>(sr, cdivD(cmul(cmulD(cmul(f, Li), fabs(vdot(wi, n))), T), pdf));
              pf |= PF_HAS_SH;
            }
          }
          again = true;
        } else if (!rp.dlSpecular && 0 + 1 < rp.maxDepth) {
          // no mirror / glass in the scene: SpecularReflect / SpecularTransmit find no specular lobe (k_shade_spec does not run)
          L = cadd(L, C3{0.f, 0.f, 0.f});
          L = cadd(L, C3{0.f, 0.f, 0.f});
        }
        stcf<F_L>(sr, L);
      } else if (stage == 0) {
        store_escaped_Le(sc, sr);
      }
      sr.u32<F_FLAGS>() = pf;
    }
    stage_loop_push(s_push, loop, q, it, false, false, (pf & PF_HAS_SH) != 0, again, slot, Q_MIS_BIT, vert);
  }
  stage_loop_end(s_push, loop, q);
}

void launch_shade_whitted(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int stage, int grid, hipStream_t s) {
  const size_t x = light_table_bytes(sc) + mat_table_bytes(sc);
  if (lightsInLds(sc) && push_stage_bytes(SHADE_BLOCK_OF(true)) + x <= 160 * 1024)
    launch_shade<k_shade_whitted<true>, SHADE_BLOCK_OF(true)>(grid, x, s, sc, rp, st, q, stage);
  else
    launch_shade<k_shade_whitted<false>, SHADE_BLOCK_OF(true)>(grid, 0, s, sc, rp, st, q, stage);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
