// dr_shade_prt.hip -- k_shade_prt: DiffusePRTIntegrator.Li (surface_integrators/diffuse_prt_integrator.dart:45-81) with
// SphericalHarmonics.ComputeDiffuseTransfer (core/spherical_harmonics.dart:557-578), one occlusion ray per slot and stage.
//
// A camera hit projects its diffuse transfer function -- visibility times the clamped cosine -- onto Terms(lmax) spherical harmonics with nSamples
// rays Ray(p, w_i, isect.rayEpsilon), w_i = UniformSampleSphere(Sample02(i, scramble)), and returns Le + Kd * clamp(sum_j c_in[j] * c[j]), c_in the
// scene's incident-light coefficients (dr_prt_project.hip).  The stage structure is k_shade_ao's: the kernel only produces and consumes rays, the
// any-hit traversal launch of the batch runner traces them, and the host (BatchRunner::stage) names the two ray indices of a stage:
//   emit == 0    sets up the camera hit: L = isect.Le(wo), p = bsdf.dgShading.p, n = FaceForward(bsdf.dgShading.nn, wo) (the SHADING normal),
//                the two rng.randomUint() of the scramble, Kd = bsdf.rho2(wo, rng, BSDF_ALL_REFLECTION) * INV_PI, c[] = 0; an escaped camera ray
//                stores the lights' Le(ray) (sampler_renderer.dart:87-92) and leaves the lists;
//   fold >= 0    folds ray `fold` in: unless the traversal found an occluder, Evaluate(w, lmax, Ylm) in f64 and for every term
//                c[j] += Spectrum(Ylm[j] * AbsDot(w, n)) / (pdf * nSamples) with the reference's f32 stores;
//   emit >= 0    queues ray `emit` -- only where Dot(w, n) > 0: the reference tests that before it traces, so such a slot queues nothing, its
//                flags say so (no PF_HAS_SH), the next stage's fold skips it, and it stays in the lists;
//   fold == nSamples - 1 (the last ray)   L += Kd * Lo.clamp().
// The folds of a slot run in increasing ray index (one per stage), so every c[j] is the reference's serial f32 sum.
//
// Draws: the two randomUint() are draws 0 and 1 of the sample's keyed in-Li stream (kind 2), in every sampler mode.  A BSDF of
// Lambertian lobes only has rho2 = R whatever StratifiedSample2D's 72 jitter draws are, and nothing draws after them, so they are skipped; the
// host refuses every other material before the render starts (dr_api.hip).
// Per-slot state: the scramble, n and Kd in words no other kernel of a PRT render touches (no MIS ray, no throughput) -- W_SCR0, W_SCR1, W_N,
// W_KD below; F_RO = p, F_RTMIN = rayEpsilon, F_SHTMAX = infinity written once at the camera hit; the direction of the ray in flight is F_SHD
// (a Vector: three f32, exactly what Evaluate is given).  The Terms(lmax) transfer coefficients (the three channels are always equal: one f32
// per term) do not fit the path state: they live in the render's side buffer c[term][stride] (Workspace::prt; stride: the slots of this render's largest batch), which both state layouts index alike.
//
// Launch geometry is k_shade_ao's; the hit's geometry and the scramble words are the units' shared ones (dr_shade_hit.h,
// dr_li_sampling.h).  Compiled with -ffp-contract=off, like every unit.
#include "dr_kernels.h"
#include "dr_rng.h"
#include "dr_wave.h"
#include "dr_prt.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_li_sampling.h"

// per-slot words besides the scramble (dr_li_sampling.h): n (3 x f32), Kd = rho2 * INV_PI (3 x f32)
enum { W_N = F_BETA, W_KD = F_BETANEE };

__global__ void __launch_bounds__(SHADE_BLOCK_OF(true), SHADE_WAVES_OF(true))
    k_shade_prt(DScene sc, RenderParams rp, BatchState st, StageQueues q, PrtArgs a, int fold, int emit) {
  extern __shared__ __align__(16) unsigned char s_dyn[];
  PushStage& s_push = *(PushStage*)s_dyn;
  const int terms = sh_terms(a.lmax);
  // The stage loop is written out here, not dr_shade_loop.h's StageLoop: on StageLoop this kernel's 4096 fold stages took 0.4 % longer
  // (269.0 against 267.9 ms of shading, outside the parent's run-to-run spread; MEASUREMENTS.md) at unchanged registers and scratch.
  PushCtx pctx = {{0, 0, 0, 0}, 0, 0};
  const uint32_t nIn = q.nActiveIn ? *q.nActiveIn : st.nslots;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t nIter = (nIn + stride - 1) / stride;
  stage_init(s_push);
  for (uint32_t it = 0; it < nIter; ++it) {
    const uint32_t idx = it * stride + blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = idx < nIn;
    uint32_t slot = 0, pf = 0;
    bool again = false, vert = false;  // again: the slot has another stage; vert: a camera hit was set up here (statistics)
    if (valid) {
      slot = q.activeIn ? q.activeIn[idx] : idx;
      const SlotRef sr = SlotRef::of(st, slot);
      float* c = a.c + slot;  // term j: c[j * a.stride]
      bool live = emit != 0;  // (behind the camera hit's stage the lists only hold slots that hit)
      F3 n;
      uint32_t scramble[2];
      if (emit == 0) {
        const int prim = sr.i32<F_HPRIM>();
        if (prim >= 0) {
          const HitRec h = hit_rec(sc, (uint32_t)prim);
          const Tri& tr = h.tr;
          const F3 o = ld3f<F_RO>(sr), d = ld3f<F_RD>(sr);
          const F3 wo = vneg(d);
          const double t = sr.f64<F_HT>();
          DGeo dg, dgs;
          hit_geometry(sc, h, o, d, t, &dg, &dgs);
          stcf<F_L>(sr, cadd(C3{0.f, 0.f, 0.f}, hit_Le(sc.lights, tr, dg.nn, wo)));  // L = Spectrum(0); L += isect.Le(wo)
          const F3 p = dgs.p;                                          // bsdf.dgShading.p
          n = vdot(dgs.nn, wo) < 0.0 ? vneg(dgs.nn) : dgs.nn;          // Normal.FaceForward(bsdf.dgShading.nn, wo) (normal.dart:59-61)
          new_scramble(rp, st, slot, sr, scramble);
          // bsdf.rho2(wo, rng, BSDF_ALL_REFLECTION) * INV_PI for the one Lambertian lobe of a matte material (none when Kd is black):
          // ret = Spectrum(0) + R (bsdf.dart:232-247, lambertian.dart:39-41)
          const C3 R = clamp0(sc.mats[4 * (size_t)tr.mat]);            // Kd.evaluate(dgs).clamp() (matte_material.dart:54)
          const C3 rho = cblack(R) ? C3{0.f, 0.f, 0.f} : cadd(C3{0.f, 0.f, 0.f}, R);
          stcf<W_KD>(sr, cmulD(rho, DR_INV_PI));
          st3f<F_RO>(sr, p);  // Ray(p, w, rayEpsilon): infinite extent
          sr.f64<F_RTMIN>() = ray_epsilon(h.isQuad, t);
          sr.f64<F_SHTMAX>() = DR_INF;
          st3f<W_N>(sr, n);
          for (int j = 0; j < terms; ++j) c[(size_t)j * a.stride] = 0.f;  // c_transfer[i] = Spectrum(0)
          live = vert = true;
        } else {
          store_escaped_Le(sc, sr);
        }
      } else {
        n = ld3f<W_N>(sr);
        load_scramble(sr, scramble);
      }
      if (live) {
        // ray `fold`, if the previous stage queued it and nothing stopped it: `Dot(w, n) > 0 && !scene.intersectP(...)`
        if (fold >= 0 && (sr.u32<F_FLAGS>() & PF_HAS_SH) && sr.i32<F_SHOCC>() == 0) {
          const F3 w = ld3f<F_SHD>(sr);
          double Ylm[DR_SH_MAX_TERMS];
          sh_evaluate((double)w.x, (double)w.y, (double)w.z, a.lmax, a.K, Ylm);
          const double absdot = fabs(vdot(w, n));
          const double den = (1.0 / (4.0 * DR_PI)) * a.nSamples;  // pdf * nSamples, pdf = UniformSpherePdf() (montecarlo.dart:122-124)
          for (int j = 0; j < terms; ++j) {
            const float s = (float)(Ylm[j] * absdot);            // new Spectrum(Ylm[j] * AbsDot(w, n))
            const float term = (float)((double)s / den);         //   / (pdf * nSamples)
            c[(size_t)j * a.stride] = c[(size_t)j * a.stride] + term;  // c_transfer[j] +=
          }
        }
        if (emit >= 0) {
          double u[2];
          Sample02((uint32_t)emit, scramble, u);
          const F3 w = UniformSampleSphere(u[0], u[1]);
          if (vdot(w, n) > 0.0) {
            st3f<F_SHD>(sr, w);
            pf = PF_HAS_SH;
          }
        }
        if (fold == a.nSamples - 1) {
          C3 Lo = C3{0.f, 0.f, 0.f};
          for (int j = 0; j < terms; ++j) {
            const float cj = c[(size_t)j * a.stride];
            Lo = cadd(Lo, cmul(C3{a.cin[3 * j], a.cin[3 * j + 1], a.cin[3 * j + 2]}, C3{cj, cj, cj}));  // Lo += c_in[i] * c_transfer[i]
          }
          stcf<F_L>(sr, cadd(ldcf<F_L>(sr), cmul(ldcf<W_KD>(sr), clamp0_poszero(Lo))));  // L + Kd * Lo.clamp()
        } else {
          again = true;
        }
      }
      sr.u32<F_FLAGS>() = pf;
    }
    stage_push(s_push, pctx, false, false, (pf & PF_HAS_SH) != 0, again, slot, Q_MIS_BIT, vert);
    if (pctx.iters == DR_PUSH_ITERS || it + 1 == nIter)
      stage_flush(s_push, pctx, q.closestQ, q.nClosest, q.anyQ, q.nAny, q.activeOut, q.nActiveOut, &q.ctr->shade_cont);
  }
  stage_finish(s_push, pctx, q.closestQ, q.anyQ, q.activeOut, &q.ctr->shade_cont);
  shade_count(s_push, q.ctr, nIn);
}

void launch_shade_prt(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, const PrtArgs& a, int fold, int emit, int grid,
                      hipStream_t s) {
  launch_shade<k_shade_prt, SHADE_BLOCK_OF(true)>(grid, 0, s, sc, rp, st, q, a, fold, emit);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
