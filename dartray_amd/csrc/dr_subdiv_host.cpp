// dr_subdiv_host.cpp -- LoopSubdivision on the host (shapes/loop_subdivision.dart:23-516): dr_loop_subdivide, and
// what the device builder (dr_subdiv_device.hip) starts from.
//
//   sd_prepare        the constructor (:30-92) on flat arrays: startFace, the neighbours across every edge (from the sorted list of
//                     unordered vertex pairs instead of the reference's map of maps), boundary / regular, the refusals -- every input the
//                     reference crashes or loops on --, the sizes of every level and the trigonometric table of the tangents
//   dr_loop_subdivide refine() (:99-308) as serial loops over the per-element rules of dr_subdiv.h
//
// Runs without a GPU: the fallback, and the device builder's checker (the two write the same bytes).  Nothing here needs the HIP
// runtime, so the file also builds as plain C++ (the sanitizer check of tests/subdiv_host_check.cpp).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dartray_hip.h"

#include "dr_subdiv.h"

namespace {

const uint64_t kLimit = 1ull << 31;

struct EdgeSlot {
  uint32_t lo, hi, slot;  // the unordered pair and the (face, k) slot that names it
};

}  // namespace

int sd_prepare(const char* who, const uint32_t* indices, uint64_t nfaces, const float* P, uint64_t nverts, int32_t nlevels, SdLevel0& out) {
  const std::string w = std::string(who) + ": ";
  if (nlevels < 0) return dr_fail(DR_ERR_INVALID, w + "nlevels is negative");
  if (!indices || !P || nfaces == 0 || nverts == 0) return dr_fail(DR_ERR_INVALID, w + "the control mesh is empty");
  if (nfaces >= kLimit / 3 || nverts >= kLimit) return dr_fail(DR_ERR_UNSUPPORTED, w + "the refined mesh has 2^31 or more faces or vertices");
  const uint32_t nf = (uint32_t)nfaces, nv = (uint32_t)nverts;
  for (uint64_t i = 0; i < 3 * nfaces; ++i)
    if (indices[i] >= nverts) return dr_fail(DR_ERR_INVALID, w + "a vertex index is out of range");
  for (uint32_t j = 0; j < nf; ++j) {
    const uint32_t* v = indices + 3 * (size_t)j;
    if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) return dr_fail(DR_ERR_INVALID, w + "a face repeats a vertex");
  }
  out.faceV.assign(indices, indices + 3 * (size_t)nf);
  out.faceF.assign(3 * (size_t)nf, DR_SD_NONE);
  out.vertStart.assign(nv, DR_SD_NONE);
  out.vertFlags.assign(nv, 0);
  std::vector<uint32_t> nFacesOf(nv, 0u);
  for (uint32_t j = 0; j < nf; ++j)
    for (int k = 0; k < 3; ++k) {
      out.vertStart[indices[3 * (size_t)j + k]] = (int32_t)j;  // every assignment overwrites the one before (:39-49)
      ++nFacesOf[indices[3 * (size_t)j + k]];
    }
  for (uint32_t v = 0; v < nv; ++v)
    if (out.vertStart[v] < 0) return dr_fail(DR_ERR_INVALID, w + "a vertex is named by no face");

  // neighbours: the slots that name one unordered pair lie side by side in the sorted list
  std::vector<EdgeSlot> es(3 * (size_t)nf);
  for (uint32_t s = 0; s < 3 * nf; ++s) {
    const uint32_t a = indices[s], b = indices[3 * (s / 3) + (s % 3 + 1) % 3];
    es[s] = EdgeSlot{std::min(a, b), std::max(a, b), s};
  }
  std::sort(es.begin(), es.end(), [](const EdgeSlot& x, const EdgeSlot& y) {
    return x.lo != y.lo ? x.lo < y.lo : (x.hi != y.hi ? x.hi < y.hi : x.slot < y.slot);
  });
  uint64_t nedges = 0;
  for (size_t i = 0; i < es.size();) {
    size_t e = i + 1;
    while (e < es.size() && es[e].lo == es[i].lo && es[e].hi == es[i].hi) ++e;
    if (e - i > 2) return dr_fail(DR_ERR_INVALID, w + "an edge is shared by more than two faces");
    if (e - i == 2) {
      const uint32_t s0 = es[i].slot, s1 = es[i + 1].slot;
      if (indices[s0] == indices[s1]) return dr_fail(DR_ERR_INVALID, w + "two faces traverse a shared edge in the same direction");
      out.faceF[s0] = (int32_t)(s1 / 3);
      out.faceF[s1] = (int32_t)(s0 / 3);
    }
    ++nedges;
    i = e;
  }

  // boundary, valence, regular (:74-92); a vertex whose walk does not meet all of its faces has more than one fan
  SdMesh m{out.faceV.data(), out.faceF.data(), out.vertStart.data(), out.vertFlags.data(), P, nf, nv};
  uint32_t maxValence = 6;
  std::vector<int> valenceOf(nv);
  for (uint32_t v = 0; v < nv; ++v) {
    const int32_t start = out.vertStart[v];
    int32_t f = start;
    uint32_t met = 1;
    while ((f = sd_next_face(m, f, sd_vnum(m, f, (int32_t)v))) >= 0 && f != start && met <= nFacesOf[v]) ++met;
    const bool boundary = f < 0;
    if (boundary) {
      f = start;
      while ((f = sd_prev_face(m, f, sd_vnum(m, f, (int32_t)v))) >= 0 && met <= nFacesOf[v]) ++met;
    }
    if (met != nFacesOf[v]) return dr_fail(DR_ERR_INVALID, w + "the faces of a vertex do not form one fan");
    const uint32_t valence = boundary ? met + 1 : met;
    const bool regular = boundary ? valence == 4 : valence == 6;
    out.vertFlags[v] = (uint8_t)((boundary ? DR_SD_BOUNDARY : 0u) | (regular ? DR_SD_REGULAR : 0u));
    valenceOf[v] = (int)valence;
    maxValence = std::max(maxValence, valence);
  }

  // every level's sizes: a level turns a face into four, keeps its vertices, adds one per edge, splits every edge and adds three per face
  out.nf.assign(1, nf);
  out.nv.assign(1, nv);
  out.ne.assign(1, nedges);
  for (int32_t l = 0; l < nlevels; ++l) {
    const uint64_t f = out.nf.back(), v = out.nv.back(), e = out.ne.back();
    if (4 * f >= kLimit || v + e >= kLimit) return dr_fail(DR_ERR_UNSUPPORTED, w + "the refined mesh has 2^31 or more faces or vertices");
    out.nf.push_back(4 * f);
    out.nv.push_back(v + e);
    out.ne.push_back(2 * e + 3 * f);
  }

  // The tangents' weights (:258-259, :272-275) with the C library's cos / sin, one row per distinct valence.  Subdivision keeps a
  // vertex's valence and adds regular vertices only, so the control mesh's valences and the interior 6 are all the final mesh has.
  out.trigInterior.assign(maxValence + 1, DR_SD_NO_ROW);
  out.trigBoundary.assign(maxValence + 1, DR_SD_NO_ROW);
  out.trigW.clear();
  auto addInterior = [&](int valence) {
    if (out.trigInterior[valence] != DR_SD_NO_ROW) return;
    out.trigInterior[valence] = (uint32_t)out.trigW.size();
    for (int k = 0; k < valence; ++k) {
      const double a = 2.0 * M_PI * k / valence;
      out.trigW.push_back(std::cos(a));
      out.trigW.push_back(std::sin(a));
    }
  };
  addInterior(6);
  for (uint32_t v = 0; v < nv; ++v) {
    const int valence = valenceOf[v];
    if (!(out.vertFlags[v] & DR_SD_BOUNDARY)) {
      addInterior(valence);
    } else if (valence >= 5 && out.trigBoundary[valence] == DR_SD_NO_ROW) {
      out.trigBoundary[valence] = (uint32_t)out.trigW.size();
      const double theta = M_PI / (valence - 1);
      out.trigW.push_back(std::sin(theta));
      for (int k = 1; k < valence - 1; ++k) out.trigW.push_back((2 * std::cos(theta) - 2) * std::sin(k * theta));
    }
  }
  return DR_OK;
}

int sd_check_outputs(const char* who, const SdLevel0& l0, float* P_out, float* N_out, uint32_t* indices_out, uint64_t vert_cap,
                     uint64_t face_cap, uint64_t* nverts_out, uint64_t* nfaces_out, bool* done) {
  *done = true;
  if (nverts_out) *nverts_out = l0.nv.back();
  if (nfaces_out) *nfaces_out = l0.nf.back();
  if (!P_out && !N_out && !indices_out) return DR_OK;  // the size query
  if (!P_out || !N_out || !indices_out) return dr_fail(DR_ERR_INVALID, std::string(who) + ": P_out, N_out and indices_out are all set or all null");
  if (vert_cap < l0.nv.back() || face_cap < l0.nf.back()) return dr_fail(DR_ERR_INVALID, std::string(who) + ": the output buffers are too small");
  *done = false;
  return DR_OK;
}

extern "C" int dr_loop_subdivide(const uint32_t* indices, uint64_t nfaces, const float* P, uint64_t nverts, int32_t nlevels, float* P_out,
                                 float* N_out, uint32_t* indices_out, uint64_t vert_cap, uint64_t face_cap, uint64_t* nverts_out,
                                 uint64_t* nfaces_out) {
  SdLevel0 l0;
  int rc = sd_prepare("dr_loop_subdivide", indices, nfaces, P, nverts, nlevels, l0);
  if (rc != DR_OK) return rc;
  bool done = false;
  rc = sd_check_outputs("dr_loop_subdivide", l0, P_out, N_out, indices_out, vert_cap, face_cap, nverts_out, nfaces_out, &done);
  if (rc != DR_OK || done) return rc;

  std::vector<int32_t> faceV = std::move(l0.faceV), faceF = std::move(l0.faceF), vertStart = std::move(l0.vertStart);
  std::vector<uint8_t> vertFlags = std::move(l0.vertFlags);
  std::vector<float> pos(P, P + 3 * (size_t)nverts);
  for (int32_t l = 0; l < nlevels; ++l) {
    const uint32_t nf = (uint32_t)l0.nf[l], nv = (uint32_t)l0.nv[l], nv2 = (uint32_t)l0.nv[l + 1];
    const SdMesh m{faceV.data(), faceF.data(), vertStart.data(), vertFlags.data(), pos.data(), nf, nv};
    std::vector<int32_t> faceV2(12 * (size_t)nf), faceF2(12 * (size_t)nf), vertStart2(nv2), edgeVert(3 * (size_t)nf, DR_SD_NONE);
    std::vector<uint8_t> vertFlags2(nv2);
    std::vector<float> pos2(3 * (size_t)nv2);
    for (uint32_t v = 0; v < nv; ++v) {  // even vertices: old-vertex order (:109-138)
      sd_store(pos2.data(), v, sd_even(m, (int32_t)v));
      vertFlags2[v] = vertFlags[v];
    }
    uint32_t next = nv;  // odd vertices: in order of first appearance (:143-172)
    for (uint32_t slot = 0; slot < 3 * nf; ++slot) {
      if (!sd_creates(m, slot)) continue;
      edgeVert[slot] = (int32_t)next;
      sd_store(pos2.data(), next, sd_odd(m, slot));
      vertFlags2[next] = (uint8_t)(DR_SD_REGULAR | (faceF[slot] < 0 ? DR_SD_BOUNDARY : 0u));
      vertStart2[next] = (int32_t)(4 * (slot / 3) + 3);
      ++next;
    }
    if (next != nv2) return dr_fail(DR_ERR_INVALID, "dr_loop_subdivide: internal error: a level's vertex count is not the predicted one");
    for (uint32_t j = 0; j < nf; ++j) sd_topology(m, edgeVert.data(), j, faceV2.data(), faceF2.data(), vertStart2.data());
    faceV.swap(faceV2);
    faceF.swap(faceF2);
    vertStart.swap(vertStart2);
    vertFlags.swap(vertFlags2);
    pos.swap(pos2);
  }

  const uint32_t nf = (uint32_t)l0.nf.back(), nv = (uint32_t)l0.nv.back();
  SdMesh m{faceV.data(), faceF.data(), vertStart.data(), vertFlags.data(), pos.data(), nf, nv};
  for (uint32_t v = 0; v < nv; ++v) sd_store(P_out, v, sd_limit(m, (int32_t)v));  // all limits from the pre-limit positions (:228-239)
  m.P = P_out;
  const SdTrig trig{l0.trigInterior.data(), l0.trigBoundary.data(), l0.trigW.data()};
  for (uint32_t v = 0; v < nv; ++v) sd_store(N_out, v, sd_normal(m, trig, (int32_t)v));
  for (size_t i = 0; i < 3 * (size_t)nf; ++i) indices_out[i] = (uint32_t)faceV[i];
  return DR_OK;
}
