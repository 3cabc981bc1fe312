// dr_nurbs_host.cpp -- Nurbs.refine on the host (shapes/nurbs.dart:76-154): dr_nurbs_dice, and what the device builder
// (dr_nurbs_device.hip) starts from.
//
//   nb_prepare     the refusals -- every input on which the reference indexes outside a list or loops --, the homogeneous copy of a
//                  'P' control net (:97-107) and the effective dice rates
//   dr_nurbs_dice  the double loop :109-122 and the index loop :132-142 as serial loops over the rules of dr_nurbs.h
//
// Runs without a GPU: the fallback, and the device builder's checker.  Nothing here needs the HIP runtime, so the file also builds as
// plain C++ (the sanitizer check of tests/nurbs_host_check.cpp).
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dartray_hip.h"

#include "dr_nurbs.h"

namespace {

// "" or what is wrong with one direction's knots and range
std::string check_direction(const char* d, int32_t n, int32_t order, const float* knot, float t0, float t1) {
  const std::string D(d);
  if (order < 2 || order > DR_NURBS_MAX_ORDER) return D + "order is below 2 or above DR_NURBS_MAX_ORDER (8)";
  if (n < order) return "n" + D + " is below " + D + "order";
  if (!knot) return D + "knots is null";
  for (int32_t i = 0; i < n + order; ++i) {
    if (!std::isfinite(knot[i])) return "a " + D + " knot is not finite";
    if (i > 0 && knot[i] < knot[i - 1]) return "the " + D + " knot vector decreases";
  }
  const float lo = knot[order - 1], hi = knot[n];
  if (!(t0 >= lo && t0 <= hi && t1 >= lo && t1 <= hi)) return D + "0 or " + D + "1 is outside [" + D + "knots[" + D + "order - 1], " + D + "knots[n" + D + "]]";
  return "";
}

}  // namespace

int nb_prepare(const char* who, const DrNurbsPatch* patch, NbPrepared& out) {
  const std::string w = std::string(who) + ": ";
  if (!patch) return dr_fail(DR_ERR_INVALID, w + "the patch is null");
  std::string bad = check_direction("u", patch->nu, patch->uorder, patch->uknots, patch->u0, patch->u1);
  if (bad.empty()) bad = check_direction("v", patch->nv, patch->vorder, patch->vknots, patch->v0, patch->v1);
  if (!bad.empty()) return dr_fail(DR_ERR_INVALID, w + bad);
  const uint64_t npt = (uint64_t)patch->nu * (uint64_t)patch->nv;
  if (npt > (1ull << 24)) return dr_fail(DR_ERR_INVALID, w + "nu * nv is above 2^24");
  if (!patch->cp) return dr_fail(DR_ERR_INVALID, w + "cp is null");
  const uint32_t diceu = patch->diceu ? patch->diceu : 30u, dicev = patch->dicev ? patch->dicev : 30u;
  if (diceu < 2 || dicev < 2 || diceu > 4096 || dicev > 4096 || (uint64_t)diceu * dicev > (1ull << 22))
    return dr_fail(DR_ERR_INVALID, w + "diceu or dicev is below 2 or above 4096, or diceu * dicev is above 2^22");
  out.Pw.resize(4 * (size_t)npt);
  if (patch->homogeneous) {
    out.Pw.assign(patch->cp, patch->cp + 4 * (size_t)npt);
  } else {
    for (size_t i = 0; i < (size_t)npt; ++i) {  // :100-106
      out.Pw[4 * i] = patch->cp[3 * i];
      out.Pw[4 * i + 1] = patch->cp[3 * i + 1];
      out.Pw[4 * i + 2] = patch->cp[3 * i + 2];
      out.Pw[4 * i + 3] = 1.0f;
    }
  }
  out.view = NbPatch{patch->uknots, patch->vknots, out.Pw.data(), patch->nu, patch->uorder, patch->nv, patch->vorder,
                     patch->u0,     patch->u1,     patch->v0,     patch->v1, diceu,         dicev};
  out.nverts = (uint64_t)diceu * dicev;
  out.ntris = 2ull * (diceu - 1) * (dicev - 1);
  return DR_OK;
}

int nb_check_outputs(const char* who, const NbPrepared& p, const float* P_out, const float* N_out, const float* uv_out,
                     const uint32_t* indices_out, uint64_t vert_cap, uint64_t tri_cap, uint64_t* nverts, uint64_t* ntris, bool* done) {
  *done = true;
  if (!P_out && !N_out && !uv_out && !indices_out) {  // the size query
    if (nverts) *nverts = p.nverts;
    if (ntris) *ntris = p.ntris;
    return DR_OK;
  }
  if (!P_out || !N_out || !uv_out || !indices_out)
    return dr_fail(DR_ERR_INVALID, std::string(who) + ": P_out, N_out, uv_out and indices_out are all set or all null");
  if (vert_cap < p.nverts || tri_cap < p.ntris) return dr_fail(DR_ERR_INVALID, std::string(who) + ": the output buffers are too small");
  if (nverts) *nverts = p.nverts;
  if (ntris) *ntris = p.ntris;
  *done = false;
  return DR_OK;
}

extern "C" int dr_nurbs_dice(const DrNurbsPatch* patch, float* P_out, float* N_out, float* uv_out, uint32_t* indices_out, uint64_t vert_cap,
                             uint64_t tri_cap, uint64_t* nverts, uint64_t* ntris) {
  NbPrepared prep;
  int rc = nb_prepare("dr_nurbs_dice", patch, prep);
  if (rc != DR_OK) return rc;
  bool done = false;
  rc = nb_check_outputs("dr_nurbs_dice", prep, P_out, N_out, uv_out, indices_out, vert_cap, tri_cap, nverts, ntris, &done);
  if (rc != DR_OK || done) return rc;
  const NbPatch& p = prep.view;
  for (uint32_t v = 0; v < p.dicev; ++v)
    for (uint32_t u = 0; u < p.diceu; ++u) {
      const size_t pi = (size_t)v * p.diceu + u;
      const NbVertex o = nb_vertex(p, u, v);
      for (int c = 0; c < 3; ++c) {
        P_out[3 * pi + c] = o.P[c];
        N_out[3 * pi + c] = o.N[c];
      }
      uv_out[2 * pi] = o.uv[0];
      uv_out[2 * pi + 1] = o.uv[1];
    }
  for (uint32_t v = 0; v + 1 < p.dicev; ++v)
    for (uint32_t u = 0; u + 1 < p.diceu; ++u) nb_quad(p.diceu, u, v, indices_out + 6 * ((size_t)v * (p.diceu - 1) + u));
  return DR_OK;
}
