// dr_subdiv.h -- Loop subdivision (shapes/loop_subdivision.dart:23-516): the flat mesh of one level and the
// per-element rules, written once for the host builder (dr_subdiv_host.cpp) and the device builder (dr_subdiv_device.hip).
//
// A level is five flat arrays instead of the reference's _SDVertex / _SDFace objects: faceV[nf][3] (vertex numbers), faceF[nf][3]
// (the neighbour across edge (v[k], v[(k+1)%3]), DR_SD_NONE for a boundary edge), vertStart[nv] (startFace), vertFlags[nv]
// (boundary / regular) and P[nv][3].  Every function below is one element's share of a loop of the reference: it reads one level
// and returns what that element writes, so a serial loop and a kernel with one lane per element produce the same bytes.
//
// Arithmetic: Point / Vector / Normal store f32, every operator computes in f64 and rounds each component once (vector.dart:27,
// :57-74; point.dart:35-45) -- sd_mul / sd_add / sd_sub below; a compound line keeps the reference's operator order.  The units
// that include this header are compiled with -ffp-contract=off.
#ifndef DR_SUBDIV_H
#define DR_SUBDIV_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DR_SD_HD __host__ __device__ inline
#else
#define DR_SD_HD inline
#endif

#define DR_SD_NONE (-1)
#define DR_SD_BOUNDARY 1u  // vertFlags bits: _SDVertex.boundary
#define DR_SD_REGULAR 2u   //                 _SDVertex.regular (interior valence 6, boundary valence 4)
#define DR_SD_NO_ROW 0xFFFFFFFFu

struct SdMesh {
  const int32_t* faceV;
  const int32_t* faceF;
  const int32_t* vertStart;
  const uint8_t* vertFlags;
  const float* P;
  uint32_t nf, nv;
};

// The trigonometric weights of the tangents (:258-259, :272-275), computed by the host per distinct valence (sd_prepare): they depend
// on (valence, k) alone.  interior[valence] / boundary[valence]: offset of the valence's row in w, DR_SD_NO_ROW where no vertex of the
// mesh has it.  An interior row is valence pairs (cos(2 pi k / valence), sin(2 pi k / valence)); a boundary row (valence >= 5) is
// sin(theta) followed by the weights (2 cos(theta) - 2) * sin(k theta) of k = 1 .. valence - 2, theta = pi / (valence - 1).
struct SdTrig {
  const uint32_t* interior;
  const uint32_t* boundary;
  const double* w;
};

struct SdP {
  float x, y, z;
};

DR_SD_HD SdP sd_mul(SdP a, double s) { return SdP{(float)((double)a.x * s), (float)((double)a.y * s), (float)((double)a.z * s)}; }
DR_SD_HD SdP sd_add(SdP a, SdP b) {
  return SdP{(float)((double)a.x + (double)b.x), (float)((double)a.y + (double)b.y), (float)((double)a.z + (double)b.z)};
}
DR_SD_HD SdP sd_sub(SdP a, SdP b) {
  return SdP{(float)((double)a.x - (double)b.x), (float)((double)a.y - (double)b.y), (float)((double)a.z - (double)b.z)};
}
DR_SD_HD SdP sd_neg(SdP a) { return SdP{-a.x, -a.y, -a.z}; }
DR_SD_HD SdP sd_cross(SdP a, SdP b) {  // Vector.Cross (vector.dart:158-168): f64 products and differences, one f32 store
  const double ax = a.x, ay = a.y, az = a.z, bx = b.x, by = b.y, bz = b.z;
  return SdP{(float)((ay * bz) - (az * by)), (float)((az * bx) - (ax * bz)), (float)((ax * by) - (ay * bx))};
}
DR_SD_HD SdP sd_point(const SdMesh& m, int32_t v) { return SdP{m.P[3 * (size_t)v], m.P[3 * (size_t)v + 1], m.P[3 * (size_t)v + 2]}; }
DR_SD_HD void sd_store(float* P, size_t v, SdP p) {
  P[3 * v] = p.x;
  P[3 * v + 1] = p.y;
  P[3 * v + 2] = p.z;
}

// _SDFace.vnum / nextFace / prevFace / nextVert / prevVert (:463-487)
DR_SD_HD int sd_vnum(const SdMesh& m, int32_t f, int32_t v) {
  const int32_t* fv = m.faceV + 3 * (size_t)f;
  return fv[0] == v ? 0 : (fv[1] == v ? 1 : 2);
}
DR_SD_HD int32_t sd_next_face(const SdMesh& m, int32_t f, int k) { return m.faceF[3 * (size_t)f + k]; }
DR_SD_HD int32_t sd_prev_face(const SdMesh& m, int32_t f, int k) { return m.faceF[3 * (size_t)f + (k + 2) % 3]; }
DR_SD_HD SdP sd_next_vert(const SdMesh& m, int32_t f, int k) { return sd_point(m, m.faceV[3 * (size_t)f + (k + 1) % 3]); }
DR_SD_HD SdP sd_prev_vert(const SdMesh& m, int32_t f, int k) { return sd_point(m, m.faceV[3 * (size_t)f + (k + 2) % 3]); }

// The far end of the nextFace chain of a boundary vertex: where its one-ring starts (:442-447)
DR_SD_HD int32_t sd_ring_first_face(const SdMesh& m, int32_t v) {
  int32_t face = m.vertStart[v];
  for (uint32_t guard = 0; guard < m.nf; ++guard) {  // (a validated mesh ends the chain long before; a walk never outlives the face count)
    const int32_t f2 = sd_next_face(m, face, sd_vnum(m, face, v));
    if (f2 < 0) break;
    face = f2;
  }
  return face;
}

// _SDVertex.valence (:409-430).  A regular vertex needs no walk.
DR_SD_HD int sd_valence(const SdMesh& m, int32_t v) {
  const uint32_t flags = m.vertFlags[v];
  if (flags & DR_SD_REGULAR) return (flags & DR_SD_BOUNDARY) ? 4 : 6;
  const int32_t start = m.vertStart[v];
  int nf = 1;
  int32_t f = start;
  if (!(flags & DR_SD_BOUNDARY)) {
    while ((f = sd_next_face(m, f, sd_vnum(m, f, v))) != start && f >= 0 && (uint32_t)nf < m.nf) ++nf;
    return nf;
  }
  while ((f = sd_next_face(m, f, sd_vnum(m, f, v))) >= 0 && (uint32_t)nf < m.nf) ++nf;
  f = start;
  while ((f = sd_prev_face(m, f, sd_vnum(m, f, v))) >= 0 && (uint32_t)nf < m.nf) ++nf;
  return nf + 1;
}

DR_SD_HD double sd_beta(int valence) { return valence == 3 ? 3.0 / 16.0 : 3.0 / (8.0 * valence); }  // :326-331
DR_SD_HD double sd_gamma(int valence) { return 1.0 / (valence + 3.0 / (8.0 * sd_beta(valence))); }  // :356-358

// WeightOneRing (:333-343): the ring of an interior vertex, summed in ring order from startFace
DR_SD_HD SdP sd_weight_one_ring(const SdMesh& m, int32_t v, int valence, double beta) {
  SdP p = sd_mul(sd_point(m, v), 1.0 - valence * beta);
  const int32_t start = m.vertStart[v];
  int32_t face = start;
  int n = 0;
  do {
    const int k = sd_vnum(m, face, v);
    p = sd_add(p, sd_mul(sd_next_vert(m, face, k), beta));
    face = sd_next_face(m, face, k);
  } while (face != start && face >= 0 && ++n < valence);
  return p;
}

// WeightBoundary (:345-354): the two ends of the ring of a boundary vertex
DR_SD_HD SdP sd_weight_boundary(const SdMesh& m, int32_t v, double beta) {
  SdP p = sd_mul(sd_point(m, v), 1.0 - 2.0 * beta);
  int32_t face = sd_ring_first_face(m, v);
  p = sd_add(p, sd_mul(sd_next_vert(m, face, sd_vnum(m, face, v)), beta));
  SdP last = p;
  for (uint32_t guard = 0; guard < m.nf && face >= 0; ++guard) {
    const int k = sd_vnum(m, face, v);
    last = sd_prev_vert(m, face, k);
    face = sd_prev_face(m, face, k);
  }
  return sd_add(p, sd_mul(last, beta));
}

// The even child's position (:126-138)
DR_SD_HD SdP sd_even(const SdMesh& m, int32_t v) {
  const uint32_t flags = m.vertFlags[v];
  if (flags & DR_SD_BOUNDARY) return sd_weight_boundary(m, v, 1.0 / 8.0);
  if (flags & DR_SD_REGULAR) return sd_weight_one_ring(m, v, 6, 1.0 / 16.0);
  const int valence = sd_valence(m, v);
  return sd_weight_one_ring(m, v, valence, sd_beta(valence));
}

// Pushed to the limit surface (:228-235)
DR_SD_HD SdP sd_limit(const SdMesh& m, int32_t v) {
  if (m.vertFlags[v] & DR_SD_BOUNDARY) return sd_weight_boundary(m, v, 1.0 / 5.0);
  const int valence = sd_valence(m, v);
  return sd_weight_one_ring(m, v, valence, sd_gamma(valence));
}

// Does slot (j, k) create the odd vertex of its edge?  The first appearance of the edge over (j ascending, k = 0, 1, 2) (:143-151): on a
// manifold mesh the edge has no other face or one that comes later.
DR_SD_HD bool sd_creates(const SdMesh& m, uint32_t slot) {
  const int32_t f2 = m.faceF[slot];
  return f2 < 0 || (uint32_t)f2 > slot / 3u;
}

// The odd vertex of the creating slot (:160-167)
DR_SD_HD SdP sd_odd(const SdMesh& m, uint32_t slot) {
  const uint32_t j = slot / 3u;
  const int k = (int)(slot % 3u);
  const int32_t* fv = m.faceV + 3 * (size_t)j;
  const int32_t v1 = fv[k], v2 = fv[(k + 1) % 3];
  const int32_t f2 = m.faceF[slot];
  if (f2 < 0) return sd_add(sd_mul(sd_point(m, v1), 0.5), sd_mul(sd_point(m, v2), 0.5));
  SdP p = sd_add(sd_mul(sd_point(m, v1), 3.0 / 8.0), sd_mul(sd_point(m, v2), 3.0 / 8.0));
  p = sd_add(p, sd_mul(sd_point(m, fv[(k + 2) % 3]), 1.0 / 8.0));  // face.otherVert
  const int32_t* gv = m.faceV + 3 * (size_t)f2;
  const int32_t o2 = (gv[0] != v1 && gv[0] != v2) ? gv[0] : ((gv[1] != v1 && gv[1] != v2) ? gv[1] : gv[2]);
  return sd_add(p, sd_mul(sd_point(m, o2), 1.0 / 8.0));
}

// The odd vertex on edge k of face j (edgeVerts.getEdge, :214): the creating slot's entry of edgeVert -- this slot's own, or the
// neighbour's, whose edge starts where this one ends (two faces traverse a shared edge in opposite directions).
DR_SD_HD int32_t sd_edge_vert(const SdMesh& m, const int32_t* edgeVert, uint32_t j, int k) {
  const uint32_t slot = 3u * j + (uint32_t)k;
  if (sd_creates(m, slot)) return edgeVert[slot];
  const int32_t f2 = m.faceF[slot];
  return edgeVert[3 * (size_t)f2 + sd_vnum(m, f2, m.faceV[3 * (size_t)j + (k + 1) % 3])];
}

// The four children of face j, faces 4j .. 4j+3 of the next level (:183-220), and the startFace of the even children whose
// parent starts at j (:177-181).
DR_SD_HD void sd_topology(const SdMesh& m, const int32_t* edgeVert, uint32_t j, int32_t* faceV, int32_t* faceF, int32_t* vertStart) {
  const int32_t* fv = m.faceV + 3 * (size_t)j;
  const int32_t* ff = m.faceF + 3 * (size_t)j;
  int32_t ev[3];
  for (int k = 0; k < 3; ++k) ev[k] = sd_edge_vert(m, edgeVert, j, k);
  const size_t c = 4 * (size_t)j;
  for (int k = 0; k < 3; ++k) {
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    int32_t* cv = faceV + 3 * (c + k);
    int32_t* cf = faceF + 3 * (c + k);
    cv[k] = fv[k];  // the even child keeps its parent's number
    cv[k1] = ev[k];
    cv[k2] = ev[k2];
    cf[k1] = (int32_t)(c + 3);
    cf[k] = ff[k] >= 0 ? 4 * ff[k] + sd_vnum(m, ff[k], fv[k]) : DR_SD_NONE;
    cf[k2] = ff[k2] >= 0 ? 4 * ff[k2] + sd_vnum(m, ff[k2], fv[k]) : DR_SD_NONE;
    faceV[3 * (c + 3) + k] = ev[k];
    faceF[3 * (c + 3) + k] = (int32_t)(c + k1);
    if (m.vertStart[fv[k]] == (int32_t)j) vertStart[fv[k]] = (int32_t)(c + k);
  }
}

// The normal of vertex v from the limit positions m.P (:246-282): N = Cross(S, T)
DR_SD_HD SdP sd_normal(const SdMesh& m, const SdTrig& trig, int32_t v) {
  SdP S{0.f, 0.f, 0.f}, T{0.f, 0.f, 0.f};
  const int valence = sd_valence(m, v);
  if (!(m.vertFlags[v] & DR_SD_BOUNDARY)) {
    const double* row = trig.w + trig.interior[valence];
    const int32_t start = m.vertStart[v];
    int32_t face = start;
    int k = 0;
    do {
      const int kv = sd_vnum(m, face, v);
      const SdP p = sd_next_vert(m, face, kv);
      S = sd_add(S, sd_mul(p, row[2 * k]));
      T = sd_add(T, sd_mul(p, row[2 * k + 1]));
      face = sd_next_face(m, face, kv);
    } while (face != start && face >= 0 && ++k < valence);
    return sd_cross(S, T);
  }
  const SdP vp = sd_point(m, v);
  const int32_t first = sd_ring_first_face(m, v);
  const SdP r0 = sd_next_vert(m, first, sd_vnum(m, first, v));
  SdP r1 = r0, r2 = r0, r3 = r0, last = r0;
  int32_t face = first;
  for (int n = 1; n < valence && face >= 0; ++n) {
    const int kv = sd_vnum(m, face, v);
    last = sd_prev_vert(m, face, kv);
    if (n == 1) r1 = last;
    if (n == 2) r2 = last;
    if (n == 3) r3 = last;
    face = sd_prev_face(m, face, kv);
  }
  S = sd_sub(last, r0);
  if (valence == 2) {
    T = sd_sub(sd_add(r0, r1), sd_mul(vp, 2.0));
  } else if (valence == 3) {
    T = sd_sub(r1, vp);
  } else if (valence == 4) {
    T = sd_add(sd_add(sd_add(sd_add(sd_mul(r0, -1.0), sd_mul(r1, 2.0)), sd_mul(r2, 2.0)), sd_mul(r3, -1.0)), sd_mul(vp, -2.0));
  } else {
    const double* row = trig.w + trig.boundary[valence];
    T = sd_mul(sd_add(r0, last), row[0]);
    face = first;
    for (int k = 1; k < valence - 1 && face >= 0; ++k) {
      const int kv = sd_vnum(m, face, v);
      T = sd_add(T, sd_mul(sd_prev_vert(m, face, kv), row[k]));
      face = sd_prev_face(m, face, kv);
    }
    T = sd_neg(T);
  }
  return sd_cross(S, T);
}

#include <string>
#include <vector>

// What both builders start from: the validated control mesh as level 0 (the constructor, :30-92), the trigonometric table of the
// valences it has, and the sizes of every level.  dr_subdiv_host.cpp.
struct SdLevel0 {
  std::vector<int32_t> faceV, faceF, vertStart;
  std::vector<uint8_t> vertFlags;
  std::vector<uint32_t> trigInterior, trigBoundary;
  std::vector<double> trigW;
  std::vector<uint64_t> nf, nv, ne;  // faces, vertices and edges of level 0 .. nlevels
};
// DR_OK, or the refusal (dr_last_error names it; `who` prefixes the message)
int sd_prepare(const char* who, const uint32_t* indices, uint64_t nfaces, const float* P, uint64_t nverts, int32_t nlevels, SdLevel0& out);
// The arguments every entry point checks the same way, and the size query: DR_OK with *done set when the call ends here
int sd_check_outputs(const char* who, const SdLevel0& l0, float* P_out, float* N_out, uint32_t* indices_out, uint64_t vert_cap,
                     uint64_t face_cap, uint64_t* nverts_out, uint64_t* nfaces_out, bool* done);
int dr_fail(int code, const std::string& msg);  // dr_api.hip: sets dr_last_error()

#endif
