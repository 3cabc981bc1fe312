// dr_shade_probes.hip -- k_shade_probes: UseProbesIntegrator.Li (surface_integrators/use_probes_integrator.dart:90-170) of every camera hit, from a
// grid of radiance probes set on the scene (dr_scene_set_probes; baked by dr_probes.hip or read from a file).  DESIGN.md 2.18.
//
//   L = isect.Le(wo) + rho * INV_PI * clamp(sum_i c_E[i] * Ylm[i])
//   offset = bbox.offset(bsdf.dgShading.p) (a Vector: f32 stores), vox = offset * nProbes - 0.5, v = floor(vox), d = vox - v;
//   c_inp[i] = the trilinear interpolation of the eight corners' coefficients, every corner index clamped to the grid (c_inXYZ), every Lerp
//              `v1 * (1 - t) + v2 * t` on Spectrum (three f32 stores each), x first, then y, then z;
//   c_E = ConvolveCosTheta(c_inp): c_inp[Index(l, m)] * (_lambda(l) * c_costheta[l]);
//   Ylm = Evaluate(Vector.FaceForward(n, wo), lmax) into a Float32List (n = bsdf.dgShading.nn: the SHADING normal);
//   rho = bsdf.rho2(wo, rng, BSDF_ALL_REFLECTION) = R for the one Lambertian lobe of a matte material (none when Kd is black): as under diffuse
//         PRT the 72 jitter draws feed nothing, and the host refuses every other material before the render starts.
// A grid with includeDirect 0 is refused by the host (that path is UniformSampleAllLights), so nothing is traced behind the camera rays and nothing
// is queued: one launch per batch, one lane per slot, slots in order, as in k_shade_feature.  An escaped camera ray stores the lights' Le(ray).
// Compiled with -ffp-contract=off, like every unit.
#include "dr_kernels.h"
#include "dr_wave.h"
#include "dr_probes.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_shade_loop.h"

#define DR_PROBES_BLOCK 256

DR_DEV C3 probes_lerp(double t, C3 v1, C3 v2) { return cadd(cmulD(v1, 1.0 - t), cmulD(v2, t)); }  // common.dart:80-81 on Spectrum
DR_DEV int probes_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// c_inXYZ (:164-170), in floats: 3 * Terms(lmax) * offset
DR_DEV size_t probes_cell(const ProbeArgs& a, int vx, int vy, int vz) {
  vx = probes_clampi(vx, 0, a.n[0] - 1);
  vy = probes_clampi(vy, 0, a.n[1] - 1);
  vz = probes_clampi(vz, 0, a.n[2] - 1);
  return (size_t)(3 * sh_terms(a.lmax)) * ((size_t)vx + (size_t)vy * (size_t)a.n[0] + (size_t)vz * (size_t)a.n[0] * (size_t)a.n[1]);
}
DR_DEV C3 probes_ld(const float* p) { return C3{p[0], p[1], p[2]}; }

__global__ void __launch_bounds__(DR_PROBES_BLOCK) k_shade_probes(DScene sc, BatchState st, ProbeArgs a, TraceCounters* ctr) {
  __shared__ uint32_t s_hits;
  per_slot_begin(s_hits);
  // SphericalHarmonics.ConvolveCosTheta's table (spherical_harmonics.dart:529-533); lmax <= 8
  const double c_costheta[9] = {0.8862268925, 1.0233267546, 0.4954159260, 0.0000000000, -0.1107783690, 0.0000000000, 0.0499271341, 0.0000000000, -0.0285469331};
  const int terms = sh_terms(a.lmax);
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t hits = 0u;
  for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < st.nslots; slot += stride) {
    const SlotRef sr = SlotRef::of(st, slot);
    const int prim = sr.i32<F_HPRIM>();
    C3 L;
    if (prim >= 0) {
      ++hits;
      const HitRec h = hit_rec(sc, (uint32_t)prim);
      const Tri& tr = h.tr;
      const F3 o = ld3f<F_RO>(sr), d = ld3f<F_RD>(sr);
      const F3 wo = vneg(d);
      DGeo dg, dgs;
      hit_geometry(sc, h, o, d, sr.f64<F_HT>(), &dg, &dgs);
      L = cadd(C3{0.f, 0.f, 0.f}, hit_Le(sc.lights, tr, dg.nn, wo));       // L = Spectrum(0); L += isect.Le(wo)
      const F3 p = dgs.p, n = dgs.nn;
      // bbox.offset(p) (bbox.dart:193-197)
      const F3 off = f3(((double)p.x - (double)a.bmin[0]) / ((double)a.bmax[0] - (double)a.bmin[0]),
                        ((double)p.y - (double)a.bmin[1]) / ((double)a.bmax[1] - (double)a.bmin[1]),
                        ((double)p.z - (double)a.bmin[2]) / ((double)a.bmax[2] - (double)a.bmin[2]));
      const double voxx = ((double)off.x * a.n[0]) - 0.5, voxy = ((double)off.y * a.n[1]) - 0.5, voxz = ((double)off.z * a.n[2]) - 0.5;
      // (a point far outside the bounds: the corner clamp makes every index beyond the grid the same, so the floor saturates harmlessly)
      const double lim = 1.0e9;
      const double fx = floor(fmin(fmax(voxx, -lim), lim)), fy = floor(fmin(fmax(voxy, -lim), lim)), fz = floor(fmin(fmax(voxz, -lim), lim));
      const int vx = (int)fx, vy = (int)fy, vz = (int)fz;
      const double dx = voxx - fx, dy = voxy - fy, dz = voxz - fz;
      const float* b000 = a.cin + probes_cell(a, vx, vy, vz);
      const float* b100 = a.cin + probes_cell(a, vx + 1, vy, vz);
      const float* b010 = a.cin + probes_cell(a, vx, vy + 1, vz);
      const float* b110 = a.cin + probes_cell(a, vx + 1, vy + 1, vz);
      const float* b001 = a.cin + probes_cell(a, vx, vy, vz + 1);
      const float* b101 = a.cin + probes_cell(a, vx + 1, vy, vz + 1);
      const float* b011 = a.cin + probes_cell(a, vx, vy + 1, vz + 1);
      const float* b111 = a.cin + probes_cell(a, vx + 1, vy + 1, vz + 1);
      const F3 nf = vdot(n, wo) < 0.0 ? vneg(n) : n;  // Vector.FaceForward(n, wo)
      float Ylm[DR_SH_MAX_TERMS];
      sh_evaluate((double)nf.x, (double)nf.y, (double)nf.z, a.lmax, a.K, Ylm);  // a Float32List
      C3 E = C3{0.f, 0.f, 0.f};
      int l = 0;
      for (int i = 0; i < terms; ++i) {
        if ((l + 1) * (l + 1) <= i) ++l;
        const C3 c00 = probes_lerp(dx, probes_ld(b000 + 3 * i), probes_ld(b100 + 3 * i));
        const C3 c10 = probes_lerp(dx, probes_ld(b010 + 3 * i), probes_ld(b110 + 3 * i));
        const C3 c01 = probes_lerp(dx, probes_ld(b001 + 3 * i), probes_ld(b101 + 3 * i));
        const C3 c11 = probes_lerp(dx, probes_ld(b011 + 3 * i), probes_ld(b111 + 3 * i));
        const C3 c0 = probes_lerp(dy, c00, c10);
        const C3 c1 = probes_lerp(dy, c01, c11);
        const C3 cinp = probes_lerp(dz, c0, c1);
        const C3 cE = cmulD(cinp, sqrt((4.0 * DR_PI) / (2.0 * l + 1.0)) * c_costheta[l]);  // c_in[o] * (_lambda(l) * c_costheta[l])
        E = cadd(E, cmulD(cE, (double)Ylm[i]));                                            // E += c_E[i] * Ylm[i]
      }
      const C3 R = clamp0(sc.mats[4 * (size_t)tr.mat]);            // Kd.evaluate(dgs).clamp() (matte_material.dart:54)
      const C3 rho = cblack(R) ? C3{0.f, 0.f, 0.f} : cadd(C3{0.f, 0.f, 0.f}, R);
      L = cadd(L, cmul(cmulD(rho, DR_INV_PI), clamp0_poszero(E)));  // L += rho * INV_PI * E.clamp()
    } else {
      L = escaped_Le(sc, sr);
    }
    stcf<F_L>(sr, L);
    sr.u32<F_FLAGS>() = 0u;
  }
  per_slot_end(s_hits, hits, ctr, st.nslots);
}

void launch_shade_probes(const DScene& sc, const BatchState& st, const StageQueues& q, const ProbeArgs& a, int grid, hipStream_t s) {
  launch_per_slot<k_shade_probes, DR_PROBES_BLOCK>(grid, st.nslots, s, sc, st, a, q.ctr);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
