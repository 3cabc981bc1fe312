// dr_shade_gprt.hip -- k_shade_gprt and k_gprt_finish: GlossyPRTIntegrator.Li (surface_integrators/glossy_prt_integrator.dart:56-116) with
// SphericalHarmonics.ComputeTransferMatrix, MatrixVectorMultiply and Rotate (core/spherical_harmonics.dart:580-607, 674-683, 228-347).
//
// A camera hit projects its visibility onto Terms(lmax)^2 products of spherical harmonics with nSamples rays Ray(p, w_i, isect.rayEpsilon),
// w_i = UniformSampleSphere(Sample02(i, scramble)) -- EVERY ray is traced: there is no Dot(w, n) test -- and returns
// Le + clamp(sum_i (B . Rotate(T . c_in))[i] * Ylm_i(woLocal)).  The work is split in two kernels:
//   k_shade_gprt   k_shade_prt's stages and rounds.  emit == 0 sets up the camera hit: L = isect.Le(wo), p = bsdf.dgShading.p, rayEpsilon, the
//                  scramble, the shading frame; an escaped camera ray stores the lights' Le(ray) and leaves the lists.  Every stage queues ray
//                  `emit` for every live slot.  The fold does NOT touch a matrix: it records ONE visibility bit of ray `fold` in the slot's words
//                  of the side buffer bits[nSamples / 32][stride] -- at most 512 B per slot, where T at lmax 4 would be 2.5 KB rewritten per ray.
//   k_gprt_finish  once per batch behind the last fold, one 64-lane wave per slot whose camera ray hit.  Lanes own the upper-triangle elements of
//                  T (325 at lmax 4: six registers per lane; T is grey and symmetric, Ylm[j] * Ylm[k] == Ylm[k] * Ylm[j]).  Directions go in chunks
//                  of 64: lane i regenerates w_i and evaluates its f64 Ylm into LDS, then every lane walks the chunk's unoccluded samples in
//                  increasing i and adds f32(Ylm[j] * Ylm[k] / (pdf * nSamples)) to its elements -- each element is the reference's serial f32
//                  sum.  T goes to LDS; lanes < Terms form c_t = T . c_in; THREE lanes -- one per channel, not Terms lanes -- rotate: the
//                  reference's Rotate shares objects between its lists (dr_sh_glossy.h), which makes every row depend on the rows written
//                  before it, so a channel's rotation is one serial program; lanes < Terms form c_o = B . c_l while lane 63 evaluates the
//                  Float32List Ylm of woLocal; lane 0 sums and writes L.
// LDS (static, two waves to a workgroup): Ylm[64][25] f64 per wave = 12.5 KiB -- rows 25 doubles apart, an odd stride, so the 64 lanes' b64
// stores of one term fall in 64 different bank pairs; the walk reads one row by all lanes (at most 25 addresses: broadcasts) -- T[25][25] f32
// and four short vectors: 16.3 KB per wave, 32.6 KB per workgroup of the CU's 160 KiB.
//
// Draws: the two randomUint() of the scramble are draws 0 and 1 of the sample's keyed in-Li stream (kind 2), in every sampler
// mode; nothing else draws.  Per-slot state in words no other kernel of this render touches (no MIS ray, no throughput): W_SCR0, W_SCR1, W_NN
// = bsdf.nn, W_SN = bsdf.sn = Normalize(dgShading.dpdu) (tn = Cross(nn, sn) is recomputed); F_RO = p, F_RTMIN = rayEpsilon, F_SHTMAX = infinity
// written once at the camera hit; F_RD keeps the camera ray's direction (wo = -F_RD); F_SHD is the ray in flight.
//
// k_shade_gprt's launch geometry is k_shade_ao's; its stage loop, the hit's geometry and the scramble words are the units' shared ones
// (dr_shade_loop.h, dr_shade_hit.h, dr_li_sampling.h).  Compiled with -ffp-contract=off, like every unit; atan2 / sin / cos of the rotation angles are f64.
#include "dr_kernels.h"
#include "dr_rng.h"
#include "dr_wave.h"
#include "dr_prt.h"
#include "dr_gprt.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_shade_loop.h"
#include "dr_li_sampling.h"

// per-slot words besides the scramble (dr_li_sampling.h): nn (3 x f32), sn (3 x f32)
enum { W_NN = F_BETA, W_SN = F_BETANEE };

__global__ void __launch_bounds__(SHADE_BLOCK_OF(true), SHADE_WAVES_OF(true))
    k_shade_gprt(DScene sc, RenderParams rp, BatchState st, StageQueues q, GprtArgs a, int fold, int emit) {
  extern __shared__ __align__(16) unsigned char s_dyn[];
  PushStage& s_push = *(PushStage*)s_dyn;
  StageLoop loop = stage_loop_begin(s_push, st, q);
  for (uint32_t it = 0; it < loop.nIter; ++it) {
    uint32_t slot = 0, pf = 0;
    bool again = false, vert = false;  // again: the slot has another stage; vert: a camera hit was set up here (statistics)
    if (stage_loop_slot(loop, q, it, &slot)) {
      const SlotRef sr = SlotRef::of(st, slot);
      bool live = emit != 0;  // (behind the camera hit's stage the lists only hold slots that hit)
      uint32_t scramble[2];
      if (emit == 0) {
        const int prim = sr.i32<F_HPRIM>();
        if (prim >= 0) {
          const HitRec h = hit_rec(sc, (uint32_t)prim);
          const F3 o = ld3f<F_RO>(sr), d = ld3f<F_RD>(sr);
          const F3 wo = vneg(d);
          const double t = sr.f64<F_HT>();
          DGeo dg, dgs;
          hit_geometry(sc, h, o, d, t, &dg, &dgs);
          stcf<F_L>(sr, cadd(C3{0.f, 0.f, 0.f}, hit_Le(sc.lights, h.tr, dg.nn, wo)));  // L = Spectrum(0); L += isect.Le(wo)
          new_scramble(rp, st, slot, sr, scramble);
          st3f<F_RO>(sr, dgs.p);  // Ray(p, w, rayEpsilon), p = bsdf.dgShading.p: infinite extent
          sr.f64<F_RTMIN>() = ray_epsilon(h.isQuad, t);
          sr.f64<F_SHTMAX>() = DR_INF;
          st3f<W_NN>(sr, dgs.nn);                   // bsdf.dart:45-51: nn = dgShading.nn, sn = Normalize(dgShading.dpdu)
          st3f<W_SN>(sr, vnormalize(dgs.dpdu));
          a.mark[slot] = 1u;
          live = vert = true;
        } else {
          store_escaped_Le(sc, sr);
          a.mark[slot] = 0u;
        }
      } else {
        load_scramble(sr, scramble);
      }
      if (live) {
        if (fold >= 0) {  // bit fold & 31 of word fold >> 5: `!scene.intersectP(...)`; the first bit of a word sets the whole word
          const uint32_t vis = ((sr.u32<F_FLAGS>() & PF_HAS_SH) && sr.i32<F_SHOCC>() == 0) ? 1u : 0u;
          uint32_t* wp = a.bits + (size_t)(fold >> 5) * a.stride + slot;
          const uint32_t before = (fold & 31) ? *wp : 0u;
          *wp = before | (vis << (fold & 31));
        }
        if (emit >= 0) {
          double u[2];
          Sample02((uint32_t)emit, scramble, u);
          st3f<F_SHD>(sr, UniformSampleSphere(u[0], u[1]));
          pf = PF_HAS_SH;
        }
        again = fold != a.nSamples - 1;
      }
      sr.u32<F_FLAGS>() = pf;
    }
    stage_loop_push(s_push, loop, q, it, false, false, (pf & PF_HAS_SH) != 0, again, slot, Q_MIS_BIT, vert);
  }
  stage_loop_end(s_push, loop, q);
}

#define GPRT_WAVES 2
#define GPRT_EPL 6  // upper-triangle elements per lane: ceil(325 / 64)

__global__ void __launch_bounds__(64 * GPRT_WAVES) k_gprt_finish(BatchState st, GprtArgs a) {
  __shared__ double sY[GPRT_WAVES][64 * DR_GPRT_MAX_TERMS];
  __shared__ float sT[GPRT_WAVES][DR_GPRT_MAX_TERMS * DR_GPRT_MAX_TERMS];
  __shared__ float sCt[GPRT_WAVES][3 * DR_GPRT_MAX_TERMS], sCl[GPRT_WAVES][3 * DR_GPRT_MAX_TERMS], sCo[GPRT_WAVES][3 * DR_GPRT_MAX_TERMS];
  __shared__ float sYo[GPRT_WAVES][DR_GPRT_MAX_TERMS];
  const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
  const int terms = sh_terms(a.lmax), nE = terms * (terms + 1) / 2;
  // this lane's elements (j <= k), row by row: element e = lane + 64 q
  int ej[GPRT_EPL], ek[GPRT_EPL];
#pragma unroll
  for (int qi = 0; qi < GPRT_EPL; ++qi) {
    int e = lane + 64 * qi, j = 0;
    ej[qi] = ek[qi] = -1;
    if (e < nE) {
      while (e >= terms - j) {
        e -= terms - j;
        ++j;
      }
      ej[qi] = j;
      ek[qi] = j + e;
    }
  }
  const double den = (1.0 / (4.0 * DR_PI)) * a.nSamples;  // pdf * nSamples, pdf = UniformSpherePdf() (montecarlo.dart:122-124)
  double* Y = sY[wv];
  float* T = sT[wv];
  // every barrier below is reached by the whole workgroup: the loops' bounds do not depend on the wave, `active` only predicates the work
  for (uint32_t base = blockIdx.x * GPRT_WAVES; base < st.nslots; base += gridDim.x * GPRT_WAVES) {
    const uint32_t slot = base + (uint32_t)wv;
    const bool active = slot < st.nslots && a.mark[slot < st.nslots ? slot : 0u] != 0u;
    const SlotRef sr = SlotRef::of(st, active ? slot : 0u);
    uint32_t scramble[2] = {0u, 0u};
    if (active) load_scramble(sr, scramble);
    float acc[GPRT_EPL];
#pragma unroll
    for (int qi = 0; qi < GPRT_EPL; ++qi) acc[qi] = 0.f;  // T[i] = Spectrum(0)
    for (int c0 = 0; c0 < a.nSamples; c0 += 64) {
      const int i = c0 + lane;
      if (active && i < a.nSamples) {
        double u[2];
        Sample02((uint32_t)i, scramble, u);
        const F3 w = UniformSampleSphere(u[0], u[1]);
        sh_evaluate((double)w.x, (double)w.y, (double)w.z, a.lmax, a.K, Y + lane * DR_GPRT_MAX_TERMS);
      }
      __syncthreads();
      if (active) {
        uint32_t lo = a.bits[(size_t)(c0 >> 5) * a.stride + slot];
        uint32_t hi = c0 + 32 < a.nSamples ? a.bits[(size_t)((c0 >> 5) + 1) * a.stride + slot] : 0u;
        lo = wave_bcast_first(lo);
        hi = wave_bcast_first(hi);
        for (unsigned long long m = ((unsigned long long)hi << 32) | lo; m != 0ull; m &= m - 1ull) {  // the unoccluded rays, in increasing i
          const double* y = Y + (__ffsll((long long)m) - 1) * DR_GPRT_MAX_TERMS;
#pragma unroll
          for (int qi = 0; qi < GPRT_EPL; ++qi)
            if (ej[qi] >= 0) acc[qi] = acc[qi] + (float)((y[ej[qi]] * y[ek[qi]]) / den);  // T[j][k] += Spectrum((Ylm[j] * Ylm[k]) / (pdf * nSamples))
        }
      }
      __syncthreads();
    }
    if (active) {
#pragma unroll
      for (int qi = 0; qi < GPRT_EPL; ++qi)
        if (ej[qi] >= 0) {
          T[ej[qi] * terms + ek[qi]] = acc[qi];
          T[ek[qi] * terms + ej[qi]] = acc[qi];
        }
    }
    __syncthreads();
    if (active && lane < terms) {  // c_t = T . c_in (MatrixVectorMultiply: vout[i] += v[j] * M[i][j] in j order)
      for (int ch = 0; ch < 3; ++ch) {
        float v = 0.f;
        for (int j = 0; j < terms; ++j) v = v + a.cin[3 * j + ch] * T[lane * terms + j];
        sCt[wv][3 * lane + ch] = v;
      }
    }
    __syncthreads();
    F3 sn = F3{0, 0, 0}, tn = F3{0, 0, 0}, nn = F3{0, 0, 0};
    if (active && (lane < 3 || lane == 63)) {
      nn = ld3f<W_NN>(sr);
      sn = ld3f<W_SN>(sr);
      tn = vcross(nn, sn);  // bsdf.dart:45-51
    }
    if (active && lane < 3) {  // c_l = Rotate(c_t, rot): one channel per lane
      // r1, r2, nl = bsdf.localToWorld of the three axes (bsdf.dart:181-185); Matrix4x4.values stores them as columns
      const F3 r1 = f3((double)sn.x * 1.0 + (double)tn.x * 0.0 + (double)nn.x * 0.0, (double)sn.y * 1.0 + (double)tn.y * 0.0 + (double)nn.y * 0.0,
                       (double)sn.z * 1.0 + (double)tn.z * 0.0 + (double)nn.z * 0.0);
      const F3 r2 = f3((double)sn.x * 0.0 + (double)tn.x * 1.0 + (double)nn.x * 0.0, (double)sn.y * 0.0 + (double)tn.y * 1.0 + (double)nn.y * 0.0,
                       (double)sn.z * 0.0 + (double)tn.z * 1.0 + (double)nn.z * 0.0);
      const F3 nl = f3((double)sn.x * 0.0 + (double)tn.x * 0.0 + (double)nn.x * 1.0, (double)sn.y * 0.0 + (double)tn.y * 0.0 + (double)nn.y * 1.0,
                       (double)sn.z * 0.0 + (double)tn.z * 0.0 + (double)nn.z * 1.0);
      const float m16[16] = {r1.x, r2.x, nl.x, 0.f, r1.y, r2.y, nl.y, 0.f, r1.z, r2.z, nl.z, 0.f, 0.f, 0.f, 0.f, 1.f};
      double alpha, beta, gamma;
      sh_to_zyz(m16, &alpha, &beta, &gamma);
      sh_rotate_channel(&sCt[wv][lane], 3, alpha, beta, gamma, a.lmax, &sCl[wv][lane]);
    }
    if (active && lane == 63) {  // the Float32List Ylm of woLocal = bsdf.worldToLocal(wo), wo = -ray.direction
      const F3 wo = vneg(ld3f<F_RD>(sr));
      const F3 wl = f3(vdot(wo, sn), vdot(wo, tn), vdot(wo, nn));
      float Yo[DR_SH_MAX_TERMS];
      sh_evaluate((double)wl.x, (double)wl.y, (double)wl.z, a.lmax, a.K, Yo);
      for (int i = 0; i < terms; ++i) sYo[wv][i] = Yo[i];
    }
    __syncthreads();
    if (active && lane < terms) {  // c_o = B . c_l
      for (int ch = 0; ch < 3; ++ch) {
        float v = 0.f;
        for (int j = 0; j < terms; ++j) v = v + sCl[wv][3 * j + ch] * a.B[(size_t)(lane * terms + j) * 3 + ch];
        sCo[wv][3 * lane + ch] = v;
      }
    }
    __syncthreads();
    if (active && lane == 0) {
      C3 Li = C3{0.f, 0.f, 0.f};
      for (int i = 0; i < terms; ++i) Li = cadd(Li, cmulD(C3{sCo[wv][3 * i], sCo[wv][3 * i + 1], sCo[wv][3 * i + 2]}, (double)sYo[wv][i]));  // Li += c_o[i] * Ylm[i]
      stcf<F_L>(sr, cadd(ldcf<F_L>(sr), clamp0_poszero(Li)));  // L += Li.clamp()
    }
    __syncthreads();
  }
}

void launch_shade_gprt(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, const GprtArgs& a, int fold, int emit, int grid,
                       hipStream_t s) {
  launch_shade<k_shade_gprt, SHADE_BLOCK_OF(true)>(grid, 0, s, sc, rp, st, q, a, fold, emit);
}

void launch_gprt_finish(const BatchState& st, const GprtArgs& a, hipStream_t s) {
  if (st.nslots == 0) return;
  const uint32_t blocks = std::min<uint32_t>((st.nslots + GPRT_WAVES - 1) / GPRT_WAVES, 4096u);
  hipLaunchKernelGGL(k_gprt_finish, dim3(blocks), dim3(64 * GPRT_WAVES), 0, s, st, a);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
