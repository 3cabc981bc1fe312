// dr_nurbs.h -- Nurbs.refine (shapes/nurbs.dart:76-263): the rules of one dice point and of one quad, written once for
// the host builder (dr_nurbs_host.cpp) and the device builder (dr_nurbs_device.hip).  nb_vertex is one pass of the double loop :109-122
// and returns what that pass writes; nb_quad is one pass of :132-142.  A serial loop and a kernel with one lane per point produce the
// same bytes.
//
// Arithmetic: every expression is f64; a store into a Float32List (ueval, veval, uvs, Pw, iso, cpWork) or into a component of a Vector /
// Point / Normal (deriv.x/y/z, the returned Point, Vector.Cross, Normal.normalize's invScale; vector.dart:27-34, :92-97, :158-168,
// normal.dart:35-38, :55-57) rounds once to f32; the lists NurbsEvaluate returns are List<double> and do not round.  A compound line keeps
// the reference's operator order.  The units that include this header are compiled with -ffp-contract=off.
//
// The reference's text departs from the NURBS code it was ported from (pbrt-v2 shapes/nurbs.cpp) in two index expressions, and BOTH ARE
// REPAIRED here -- the only places where this header does not restate the text:
//   * :208  j = cpi + ((cpOffset + i) * cpStride): i counts FLOATS (0, 4, 8 ...), cpOffset counts POINTS.  Right while cpOffset is 0;
//           beyond the first knot span the iso call of :178 (cpi = -4 * uFirstCp, stride 1) starts at float -3 * uFirstCp and Dart
//           raises a RangeError.  Here: j = cpi + ((cpOffset * 4 + i) * cpStride).  Same index wherever the reference does not raise.
//   * :222-225  the de Boor step's left operand is cpWork[j + c], j the POINT's number.  Here: cpWork[k + c], the point's first float --
//           the B-spline recurrence.  Order 2 never enters that loop; from order 3 on the reference's output is not the surface of its
//           control net (and has a NaN normal at vertex 0), and this header's is.
#ifndef DR_NURBS_H
#define DR_NURBS_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DR_NB_HD __host__ __device__ inline
#else
#define DR_NB_HD inline
#endif

#include "../../include/dartray_hip.h"

#define DR_NB_WORK (4 * DR_NURBS_MAX_ORDER)  // floats of cpWork / iso

// A validated patch (nb_prepare): Pw is homogeneous whatever the caller gave (:97-107), dice rates are the effective ones.
struct NbPatch {
  const float* uknot;
  const float* vknot;
  const float* Pw;  // nu * nv * 4, u fastest
  int32_t nu, uorder, nv, vorder;
  float u0, u1, v0, v1;
  uint32_t diceu, dicev;
};

struct NbVertex {
  float P[3], N[3], uv[2];
};

// KnotOffset (:253-263).  A validated t never passes knot[np]; the bound keeps a walk inside the list whatever t is.
DR_NB_HD int nb_knot_offset(const float* knot, int order, int np, double t) {
  int knotOffset = order - 1;
  while (knotOffset + 1 < np && t > (double)knot[knotOffset + 1]) ++knotOffset;
  return knotOffset;
}

// NurbsEvaluate (:197-251): out = [vx, vy, vz, vw] in f64; deriv (3 floats) when not null
DR_NB_HD void nb_evaluate(int order, const float* knot, const float* cp, int cpi, int np, int cpStride, double t, float* deriv,
                          double out[4]) {
  const int knotOffset = nb_knot_offset(knot, order, np, t);
  const int cpOffset = knotOffset - order + 1;
  float cpWork[DR_NB_WORK];
  for (int i = 0; i < 4 * order; i += 4) {
    const int j = cpi + ((cpOffset * 4 + i) * cpStride);  // repaired: see the header comment
    cpWork[i] = cp[j];
    cpWork[i + 1] = cp[j + 1];
    cpWork[i + 2] = cp[j + 2];
    cpWork[i + 3] = cp[j + 3];
  }
  for (int i = 0; i < order - 2; ++i) {
    for (int j = 0, k = 0, l = 4; j < order - 1 - i; ++j, k += 4, l += 4) {
      // (left operand cpWork[k + c]: repaired, see the header comment)
      const double alpha = ((double)knot[knotOffset + 1 + j] - t) / ((double)knot[knotOffset + 1 + j] - (double)knot[knotOffset + j + 2 - order + i]);
      cpWork[k] = (float)((double)cpWork[k] * alpha + (double)cpWork[l] * (1 - alpha));
      cpWork[k + 1] = (float)((double)cpWork[k + 1] * alpha + (double)cpWork[l + 1] * (1 - alpha));
      cpWork[k + 2] = (float)((double)cpWork[k + 2] * alpha + (double)cpWork[l + 2] * (1 - alpha));
      cpWork[k + 3] = (float)((double)cpWork[k + 3] * alpha + (double)cpWork[l + 3] * (1 - alpha));
    }
  }
  const double span = (double)knot[knotOffset + 1] - (double)knot[knotOffset];
  const double alpha = ((double)knot[knotOffset + 1] - t) / span;
  const double vx = (double)cpWork[0] * alpha + (double)cpWork[4] * (1 - alpha);
  const double vy = (double)cpWork[1] * alpha + (double)cpWork[5] * (1 - alpha);
  const double vz = (double)cpWork[2] * alpha + (double)cpWork[6] * (1 - alpha);
  const double vw = (double)cpWork[3] * alpha + (double)cpWork[7] * (1 - alpha);
  if (deriv) {
    const double factor = (double)(order - 1) / span;
    const double dx = ((double)cpWork[4] - (double)cpWork[0]) * factor;
    const double dy = ((double)cpWork[5] - (double)cpWork[1]) * factor;
    const double dz = ((double)cpWork[6] - (double)cpWork[2]) * factor;
    const double dw = ((double)cpWork[7] - (double)cpWork[3]) * factor;
    deriv[0] = (float)(dx / vw - (vx * dw / (vw * vw)));
    deriv[1] = (float)(dy / vw - (vy * dw / (vw * vw)));
    deriv[2] = (float)(dz / vw - (vz * dw / (vw * vw)));
  }
  out[0] = vx;
  out[1] = vy;
  out[2] = vz;
  out[3] = vw;
}

// NurbsEvaluateSurface (:156-195) with both derivatives: the Point's three floats
DR_NB_HD void nb_evaluate_surface(const NbPatch& p, double u, double v, float P[3], float dPdu[3], float dPdv[3]) {
  float iso[DR_NB_WORK];
  double pt[4];
  const int uFirstCp = nb_knot_offset(p.uknot, p.uorder, p.nu, u) - p.uorder + 1;
  for (int i = 0, j = 0; i < p.uorder; ++i) {
    nb_evaluate(p.vorder, p.vknot, p.Pw, (uFirstCp + i) * 4, p.nv, p.nu, v, nullptr, pt);
    iso[j++] = (float)pt[0];
    iso[j++] = (float)pt[1];
    iso[j++] = (float)pt[2];
    iso[j++] = (float)pt[3];
  }
  const int vFirstCp = nb_knot_offset(p.vknot, p.vorder, p.nv, v) - p.vorder + 1;
  double Ph[4];
  nb_evaluate(p.uorder, p.uknot, iso, (-uFirstCp) * 4, p.nu, 1, u, dPdu, Ph);
  for (int i = 0, j = 0; i < p.vorder; ++i) {
    nb_evaluate(p.uorder, p.uknot, p.Pw, ((vFirstCp + i) * p.nu) * 4, p.nu, 1, u, nullptr, pt);
    iso[j++] = (float)pt[0];
    iso[j++] = (float)pt[1];
    iso[j++] = (float)pt[2];
    iso[j++] = (float)pt[3];
  }
  nb_evaluate(p.vorder, p.vknot, iso, -vFirstCp * 4, p.nv, 1, v, dPdv, pt);
  P[0] = (float)(Ph[0] / Ph[3]);
  P[1] = (float)(Ph[1] / Ph[3]);
  P[2] = (float)(Ph[2] / Ph[3]);
}

// ueval[i] / veval[i] (:85-91): Lerp(i / (dice - 1), min, max) = min * (1.0 - t) + max * t (common.dart:80-81), stored f32
DR_NB_HD float nb_eval_param(uint32_t i, uint32_t dice, float lo, float hi) {
  const double t = (double)i / (double)(dice - 1u);
  return (float)((double)lo * (1.0 - t) + (double)hi * t);
}

// One dice point (:110-121): uvs, evalPs, evalNs of pi = vi * diceu + ui
DR_NB_HD NbVertex nb_vertex(const NbPatch& p, uint32_t ui, uint32_t vi) {
  NbVertex o;
  o.uv[0] = nb_eval_param(ui, p.diceu, p.u0, p.u1);
  o.uv[1] = nb_eval_param(vi, p.dicev, p.v0, p.v1);
  float dPdu[3], dPdv[3];
  nb_evaluate_surface(p, (double)o.uv[0], (double)o.uv[1], o.P, dPdu, dPdv);
  // Normal.Normalize(Vector.Cross(dPdu, dPdv)): the cross product stored f32, then each component /= length()
  const double ax = dPdu[0], ay = dPdu[1], az = dPdu[2], bx = dPdv[0], by = dPdv[1], bz = dPdv[2];
  const float cx = (float)((ay * bz) - (az * by)), cy = (float)((az * bx) - (ax * bz)), cz = (float)((ax * by) - (ay * bx));
  const double len = sqrt((double)cx * (double)cx + (double)cy * (double)cy + (double)cz * (double)cz);
  o.N[0] = (float)((double)cx / len);
  o.N[1] = (float)((double)cy / len);
  o.N[2] = (float)((double)cz / len);
  return o;
}

// One quad's two triangles (:132-142), VN(u, v) = v * diceu + u; the quad's number is v * (diceu - 1) + u
DR_NB_HD void nb_quad(uint32_t diceu, uint32_t u, uint32_t v, uint32_t out[6]) {
  const uint32_t a = v * diceu + u, b = a + 1u, c = (v + 1u) * diceu + u + 1u, d = c - 1u;
  out[0] = a;
  out[1] = b;
  out[2] = c;
  out[3] = a;
  out[4] = c;
  out[5] = d;
}

#include <string>
#include <vector>

// What both builders start from (dr_nurbs_host.cpp): the refusals, the homogeneous control net and the effective dice rates.  `view`
// points into Pw and into the caller's knot vectors.
struct NbPrepared {
  std::vector<float> Pw;
  NbPatch view;
  uint64_t nverts, ntris;
};
// DR_OK, or the refusal (dr_last_error names it; `who` prefixes the message)
int nb_prepare(const char* who, const DrNurbsPatch* patch, NbPrepared& out);
// The output arguments every entry point checks the same way, and the size query: DR_OK with *done set when the call ends here
int nb_check_outputs(const char* who, const NbPrepared& p, const float* P_out, const float* N_out, const float* uv_out,
                     const uint32_t* indices_out, uint64_t vert_cap, uint64_t tri_cap, uint64_t* nverts, uint64_t* ntris, bool* done);
int dr_fail(int code, const std::string& msg);  // dr_api.hip: sets dr_last_error()

#endif
