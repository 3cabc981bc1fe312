// dr_scene_build.hip -- dr_scene_create / dr_scene_destroy: the host's scene description, validated and uploaded (SceneBuilder).
//
// Host logic restated from the reference where it decides WHAT is traced:
//   light tables         ShapeSet ctor (core/light/shape_set.dart:24-51), Distribution1D (core/montecarlo.dart:25-52)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "dr_host.h"
#include "dr_scene_prep.h"

using namespace dr_host;

namespace {

#define DR_PAIR_TOP_LEVELS 12  // sibling-pair records: this many levels of the tree breadth-first in front (dr_scene_create)

inline double r32(double x) { return (double)(float)x; }

// Triangle.area (shapes/triangle.dart:265-269): Vector temporaries are f32.
double host_tri_area(const float* a, const float* b, const float* c) {
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = r32((double)b[k] - (double)a[k]);
    e2[k] = r32((double)c[k] - (double)a[k]);
  }
  double cx = r32(e1[1] * e2[2] - e1[2] * e2[1]);
  double cy = r32(e1[2] * e2[0] - e1[0] * e2[2]);
  double cz = r32(e1[0] * e2[1] - e1[1] * e2[0]);
  return 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
}

// DifferentialGeometry.nn of a hit on triangle (a,b,c) with the default UVs (triangle.dart:100-132,
// differential_geometry.dart:84-99) and the normal Triangle.sample returns (triangle.dart:376-381);
// the same f64-expression / f32-store arithmetic as tri_dg() in dr_device.h.
void host_tri_normals(const float* a, const float* b, const float* c, bool reverse, float nn[3], float ns[3],
                      const float* uv = nullptr) {
  static const float kDefaultUV[6] = {0.f, 0.f, 1.f, 0.f, 1.f, 1.f};  // triangle.dart:255-262
  if (!uv) uv = kDefaultUV;
  const double du1 = (double)uv[0] - (double)uv[4], du2 = (double)uv[2] - (double)uv[4];
  const double dv1 = (double)uv[1] - (double)uv[5], dv2 = (double)uv[3] - (double)uv[5];
  const double determinant = du1 * dv2 - dv1 * du2;
  double dpdu[3], dpdv[3];
  if (determinant == 0.0) {  // degenerate uv mapping: Vector.CoordinateSystem on the face normal (triangle.dart:108-127)
    double e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
      e1[k] = (double)b[k] - (double)a[k];
      e2[k] = (double)c[k] - (double)a[k];
    }
    const double e3x = (e2[1] * e1[2]) - (e2[2] * e1[1]), e3y = (e2[2] * e1[0]) - (e2[0] * e1[2]), e3z = (e2[0] * e1[1]) - (e2[1] * e1[0]);
    const double len = std::sqrt(e3x * e3x + e3y * e3y + e3z * e3z);
    const double v1[3] = {r32(e3x / len), r32(e3y / len), r32(e3z / len)};
    if (std::fabs(v1[0]) > std::fabs(v1[1])) {
      const double invLen = 1.0 / std::sqrt(v1[0] * v1[0] + v1[2] * v1[2]);
      dpdu[0] = r32(-v1[2] * invLen); dpdu[1] = 0.0; dpdu[2] = r32(v1[0] * invLen);
    } else {
      const double invLen = 1.0 / std::sqrt(v1[1] * v1[1] + v1[2] * v1[2]);
      dpdu[0] = 0.0; dpdu[1] = r32(v1[2] * invLen); dpdu[2] = r32(-v1[1] * invLen);
    }
    dpdv[0] = r32(v1[1] * dpdu[2] - v1[2] * dpdu[1]);
    dpdv[1] = r32(v1[2] * dpdu[0] - v1[0] * dpdu[2]);
    dpdv[2] = r32(v1[0] * dpdu[1] - v1[1] * dpdu[0]);
  } else {
    const double invdet = 1.0 / determinant;
    for (int k = 0; k < 3; ++k) {
      const double dp1 = r32((double)a[k] - (double)c[k]), dp2 = r32((double)b[k] - (double)c[k]);
      dpdu[k] = r32(r32(r32(dp1 * dv2) - r32(dp2 * dv1)) * invdet);
      dpdv[k] = r32(r32(r32(dp1 * -du2) + r32(dp2 * du1)) * invdet);
    }
  }
  auto crossNorm = [](const double* u, const double* v, double out[3]) {
    const double cx = r32(u[1] * v[2] - u[2] * v[1]), cy = r32(u[2] * v[0] - u[0] * v[2]), cz = r32(u[0] * v[1] - u[1] * v[0]);
    const double len = std::sqrt(cx * cx + cy * cy + cz * cz);
    out[0] = r32(cx / len); out[1] = r32(cy / len); out[2] = r32(cz / len);
  };
  double n[3];
  crossNorm(dpdu, dpdv, n);
  for (int k = 0; k < 3; ++k) nn[k] = (float)(reverse ? r32(n[k] * -1.0) : n[k]);
  double e1[3], e2[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = r32((double)b[k] - (double)a[k]);
    e2[k] = r32((double)c[k] - (double)a[k]);
  }
  crossNorm(e1, e2, n);
  for (int k = 0; k < 3; ++k) ns[k] = (float)(reverse ? n[k] * -1.0 : n[k]);
}

// MIPMap.texture's resampling of an RGB image to power-of-two resolution (mipmap.dart:71-138; wrap mode TEXTURE_REPEAT, the
// InfiniteAreaLight's): a four-tap Lanczos zoom in s, then in t, every product and every partial sum a new Spectrum (f32 stores),
// the t pass clamped to [0, inf) (_clamp, :358).  Weights: _resampleWeights (:360-384) in doubles.
void resample_to_pow2(const float* img, int xres, int yres, std::vector<float>& out, int* wOut, int* hOut) {
  auto roundUpPow2 = [](int v) { v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v + 1; };  // common.dart:105-113
  struct Weight { int firstTexel; double w[4]; };
  auto lanczos = [](double x) {  // texture.dart:27-39, tau = 2
    x = std::fabs(x);
    if (x < 1.0e-5) return 1.0;
    if (x > 1.0) return 0.0;
    x *= 3.141592653589793;
    const double s = std::sin(x * 2.0) / (x * 2.0);
    return s * (std::sin(x) / x);
  };
  auto weights = [&](int oldres, int newres) {
    std::vector<Weight> wt(newres);
    const double filterwidth = 2.0;
    for (int i = 0; i < newres; ++i) {
      const double center = (i + 0.5) * oldres / newres;
      wt[i].firstTexel = (int)std::floor((center - filterwidth) + 0.5);
      for (int j = 0; j < 4; ++j) wt[i].w[j] = lanczos(((wt[i].firstTexel + j + 0.5) - center) / filterwidth);
      const double invSum = 1.0 / (wt[i].w[0] + wt[i].w[1] + wt[i].w[2] + wt[i].w[3]);
      for (int j = 0; j < 4; ++j) wt[i].w[j] *= invSum;
    }
    return wt;
  };
  auto mod = [](int a, int n) { const int r = a % n; return r < 0 ? r + n : r; };  // Dart's % is never negative for a positive divisor
  const int sPow2 = roundUpPow2(xres), tPow2 = roundUpPow2(yres);
  out.assign(3 * (size_t)sPow2 * tPow2, 0.f);
  const std::vector<Weight> sW = weights(xres, sPow2);
  for (int t = 0; t < yres; ++t)
    for (int s = 0; s < sPow2; ++s)
      for (int j = 0; j < 4; ++j) {
        const int origS = mod(sW[s].firstTexel + j, xres);
        for (int c = 0; c < 3; ++c) {
          float& dst = out[3 * ((size_t)t * sPow2 + s) + c];
          const float px = (float)((double)img[3 * ((size_t)t * xres + origS) + c] * sW[s].w[j]);
          dst = (float)((double)dst + (double)px);
        }
      }
  const std::vector<Weight> tW = weights(yres, tPow2);
  std::vector<float> work(3 * (size_t)tPow2);
  for (int s = 0; s < sPow2; ++s) {
    for (int t = 0; t < tPow2; ++t)
      for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
        for (int j = 0; j < 4; ++j) {
          const int off = mod(tW[t].firstTexel + j, yres);
          const float px = (float)((double)out[3 * ((size_t)off * sPow2 + s) + c] * tW[t].w[j]);
          acc = (float)((double)acc + (double)px);
        }
        work[3 * (size_t)t + c] = acc;
      }
    for (int t = 0; t < tPow2; ++t)
      for (int c = 0; c < 3; ++c) {
        const float v = work[3 * (size_t)t + c];
        out[3 * ((size_t)t * sPow2 + s) + c] = (v < 0.f || v == 0.f) ? 0.f : v;  // num.clamp(0.0, INFINITY): NaN stays, -0.0 -> 0.0
      }
  }
  *wOut = sPow2;
  *hOut = tPow2;
}

// dr_scene_create in units (round 6): SceneBuilder carries what the steps share -- the host's description, the scene under construction, the
// primitive tables on the device -- and every step returns DR_OK or the error it has already reported (dr_scene_create then deletes the scene).
#define TRY_SC(expr)                                                             \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) return fail(DR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
struct SceneBuilder {
  const DrSceneDesc* desc;
  DrScene* sc;
  bool hostPrep = false;           // DARTRAY_SCENE_PREP=host: the serial host loops (the reference the device code is tested against)
  std::vector<uint8_t> level;      //   their per-node levels
  uint32_t measuredDepth = 0;
  DevBuf<float> dV;                // the primitive tables on the device (the device-side validation and the gather read them)
  DevBuf<uint32_t> dI, dM;
  DevBuf<int32_t> dL;
  DevBuf<uint8_t> dR;

  int validateOnHost();
  int quadrics();
  int uploadTables();
  int pairsOnDevice();
  int pairsOnHost();
  int gatherPrimitives();
  int shadingRecords();
  int materials();
  int lights();
  int envLightTables(int envLight);
  int finish();
  int directLightingLayout();
};

int SceneBuilder::validateOnHost() {
  // Validation of the marshalled tree, independent of which kernels can use it: a foreign host's BVHAccel.nodes are
  // input, and a malformed node must come back as DR_ERR_INVALID, not as an out-of-bounds device read or an endless
  // traversal.  Children always have larger indices than their parent (first child i + 1, second child offset > i + 1:
  // the depth-first numbering of bvh_accel.dart:419-437), so every walk terminates, and one forward pass gives each
  // node's level: the height of the tree bounds the traversal stack (desc->bvh_depth == 0, "unknown", is measured here).
  level.assign(hostPrep ? desc->nnodes : 0, 0);
  if (desc->nnodes && hostPrep) {
    const DrBvhNode* N = desc->nodes;
    for (uint64_t i = 0; i < desc->nnodes; ++i) {
      if (N[i].nprims == 0) {
        if (N[i].offset <= i + 1 || N[i].offset >= desc->nnodes || N[i].axis > 2)
          return fail(DR_ERR_INVALID, "malformed BVH node (interior node: second child must follow the first sub-tree, axis 0..2)");
        const uint32_t l = (uint32_t)level[i] + 1u;
        if (l > DR_MAX_STACK) return fail(DR_ERR_UNSUPPORTED, "BVH deeper than the traversal stack");
        level[i + 1] = std::max<uint8_t>(level[i + 1], (uint8_t)l);
        level[N[i].offset] = std::max<uint8_t>(level[N[i].offset], (uint8_t)l);
        measuredDepth = std::max(measuredDepth, l);
      } else if ((uint64_t)N[i].offset + N[i].nprims > desc->ntris) {
        return fail(DR_ERR_INVALID, "leaf primitive range");
      }
    }
  }
  if (desc->bvh_depth > DR_MAX_STACK) return fail(DR_ERR_UNSUPPORTED, "BVH deeper than the traversal stack");
  if (desc->bvh_depth != 0 && desc->bvh_depth < measuredDepth)
    return fail(DR_ERR_INVALID, "bvh_depth is smaller than the tree's height (pass 0 to have it measured)");
  for (uint64_t i = 0; hostPrep && i < 3 * desc->ntris; i += 3) {
    if (desc->tri_idx[i] == DR_PRIM_QUADRIC) continue;
    for (int k = 0; k < 3; ++k)
      if (desc->tri_idx[i + k] >= desc->nverts) return fail(DR_ERR_INVALID, "vertex index out of range");
  }
  return DR_OK;
}

int SceneBuilder::quadrics() {
  // quadric shapes (sphere.dart:24-32, disk.dart:24-28): constructor-derived fields in f64
  for (uint32_t i = 0; i < desc->nquadrics; ++i) {
    if (!desc->quadrics) return fail(DR_ERR_INVALID, "quadrics missing");
    const DrQuadric& a = desc->quadrics[i];
    DQuadric q;
    memset(&q, 0, sizeof(q));
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) {
        q.o2w[4 * r + c] = a.object_to_world[4 * r + c];
        q.w2o[4 * r + c] = a.world_to_object[4 * r + c];
      }
    for (int c = 0; c < 4; ++c)
      if (a.object_to_world[12 + c] != (c == 3 ? 1.0f : 0.0f) || a.world_to_object[12 + c] != (c == 3 ? 1.0f : 0.0f))
        return fail(DR_ERR_UNSUPPORTED, "projective object transforms are not on the path");
    auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
    auto radians = [](double deg) { return (3.141592653589793 / 180.0) * deg; };  // common.dart:87-88
    q.kind = a.kind;
    if (a.kind == DR_QUADRIC_SPHERE) {
      q.radius = a.params[0];
      const double z0 = a.params[1], z1 = a.params[2];
      q.zmin = clampd(std::min(z0, z1), -q.radius, q.radius);
      q.zmax = clampd(std::max(z0, z1), -q.radius, q.radius);
      q.thetaMin = std::acos(clampd(q.zmin / q.radius, -1.0, 1.0));
      q.thetaMax = std::acos(clampd(q.zmax / q.radius, -1.0, 1.0));
      q.phiMax = radians(clampd(a.params[3], 0.0, 360.0));
    } else if (a.kind == DR_QUADRIC_DISK) {
      q.height = a.params[0];
      q.radius = a.params[1];
      q.innerRadius = a.params[2];
      q.phiMax = radians(clampd(a.params[3], 0.0, 360.0));
    } else {
      return fail(DR_ERR_INVALID, "unknown quadric kind");
    }
    sc->hostQuads.push_back(q);
  }

  return DR_OK;
}

int SceneBuilder::uploadTables() {
  // nodes: the 32-byte marshalled node is consumed as two 16-byte loads
  TRY_SC(sc->nodes.alloc(2 * desc->nnodes));
  if (desc->nnodes) TRY_SC(hipMemcpy(sc->nodes.p, desc->nodes, desc->nnodes * sizeof(DrBvhNode), hipMemcpyHostToDevice));
  // the primitive tables (gathered into 48-byte records further down; the device-side validation reads them too)
  if (desc->ntris) {
    TRY_SC(dV.alloc(3 * std::max<uint64_t>(desc->nverts, 1)));
    TRY_SC(dI.alloc(3 * desc->ntris));
    TRY_SC(dM.alloc(desc->ntris));
    TRY_SC(dL.alloc(desc->ntris));
    TRY_SC(dR.alloc(desc->ntris));
    if (desc->nverts) TRY_SC(hipMemcpy(dV.p, desc->verts, 3 * desc->nverts * sizeof(float), hipMemcpyHostToDevice));
    TRY_SC(hipMemcpy(dI.p, desc->tri_idx, 3 * desc->ntris * sizeof(uint32_t), hipMemcpyHostToDevice));
    TRY_SC(hipMemcpy(dM.p, desc->tri_material, desc->ntris * sizeof(uint32_t), hipMemcpyHostToDevice));
    TRY_SC(hipMemcpy(dL.p, desc->tri_light, desc->ntris * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return DR_OK;
}

int SceneBuilder::pairsOnDevice() {
  // sibling-pair layout for the v3 traversal (see dr_device.h): children of the k-th interior node side by side
  sc->d.pairs = nullptr;
  sc->d.npairs = 0;
  sc->d.topPairs = 0;
  sc->d.rootRef = PREF_DEAD;
  if (!hostPrep) {
    ScenePrepIn pin;
    memset(&pin, 0, sizeof(pin));
    pin.nodes = sc->nodes.p;
    pin.hostNodes = desc->nodes;
    pin.nnodes = desc->nnodes;
    pin.verts = dV.p;
    pin.nverts = desc->nverts;
    pin.triIdx = dI.p;
    pin.triMaterial = dM.p;
    pin.triLight = dL.p;
    pin.ntris = desc->ntris;
    pin.nquadrics = desc->nquadrics;
    pin.nmaterials = desc->nmaterials;
    pin.nlights = desc->nlights;
    pin.wantPairs = desc->nnodes && desc->ntris < (1ull << 26) && desc->nquadrics == 0;  // only the v2 kernel tests quadrics
    pin.topLevels = DR_PAIR_TOP_LEVELS;
    if (pin.wantPairs) {
      pin.pairsCap = desc->nnodes / 2 + 1;  // a binary tree of n nodes has (n - 1) / 2 interior ones
      TRY_SC(sc->pairs.alloc(4 * pin.pairsCap));
      pin.pairsOut = sc->pairs.p;
    }
    ScenePrepOut pout;
    const int prc = scene_prepare_device(pin, &pout);
    if (prc != DR_OK) return fail(prc, pout.message);
    measuredDepth = pout.depth;
    if (desc->bvh_depth != 0 && desc->bvh_depth < measuredDepth)
      return fail(DR_ERR_INVALID, "bvh_depth is smaller than the tree's height (pass 0 to have it measured)");
    if (pout.pairsOk) {
      const DrBvhNode& r = desc->nodes[0];
      sc->d.pairs = sc->pairs.p;
      sc->d.npairs = pout.npairs;
      sc->d.topPairs = pout.topPairs;
      sc->d.rootRef = r.nprims ? (PREF_LEAF | ((uint32_t)r.nprims << 26) | r.offset) : ((uint32_t)r.axis << 29);  // (the root's pair is slot 0 in either order)
    } else {
      sc->pairs.release();
    }
  }
  sc->bvhDepth = std::max(desc->bvh_depth, measuredDepth);  // (a caller may pass a bound larger than the height)
  if (desc->nnodes && sc->bvhDepth == 0) sc->bvhDepth = 1;  // a single leaf: "known, no stack needed"
  return DR_OK;
}

// The serial reference of scene_prepare_device (DARTRAY_SCENE_PREP=host): pair records in the same memory order, the union check.
int SceneBuilder::pairsOnHost() {
  if (desc->nnodes && hostPrep) {
    const DrBvhNode* N = desc->nodes;
    bool ok = desc->ntris < (1ull << 26) && desc->nquadrics == 0;  // only the v2 kernel tests quadrics
    std::vector<uint32_t> pairIndex(desc->nnodes, 0);
    uint32_t np = 0;
    for (uint64_t i = 0; i < desc->nnodes; ++i) {
      if (N[i].nprims == 0) {
        if (i + 1 >= desc->nnodes || N[i].offset >= desc->nnodes || N[i].axis > 2) return fail(DR_ERR_INVALID, "malformed BVH node");
        pairIndex[i] = np++;
      } else if (N[i].nprims > 31) {
        ok = false;  // packed references carry at most 31 primitives per leaf; fall back to the v2 kernel
      }
    }
    // Memory order of the pair records (results never depend on it -- the references are explicit): the top DR_PAIR_TOP_LEVELS levels
    // breadth-first (3 774 records = 236 KiB on C4), then every other interior node in depth-first (= node index) order, so a sub-tree
    // below the top is one contiguous run (round 4: C4 closest-hit -1 %, any-hit -3.5 % against plain depth-first; the other orders
    // that were tried -- sibling lines, padded records, van Emde Boas treelets -- are experiments/r06_runtime_switches.diff).
    {
      std::vector<uint32_t> slotOf(desc->nnodes, 0);
      uint32_t slots = 0;
      std::vector<uint32_t> top;
      for (uint64_t i = 0; i < desc->nnodes; ++i)
        if (N[i].nprims == 0 && level[i] < DR_PAIR_TOP_LEVELS) top.push_back((uint32_t)i);
      std::stable_sort(top.begin(), top.end(), [&](uint32_t a, uint32_t b) { return level[a] < level[b]; });
      for (uint32_t i : top) slotOf[i] = slots++;
      sc->d.topPairs = slots;
      for (uint64_t i = 0; i < desc->nnodes; ++i)
        if (N[i].nprims == 0 && level[i] >= DR_PAIR_TOP_LEVELS) slotOf[i] = slots++;
      if (slots) {
        pairIndex.swap(slotOf);
        np = slots;
      }
    }
    if (np >= (1u << 29)) ok = false;
    // The v3 kernel re-derives a node's own box when it needs the literal test: an interior node's bounds
    // must be the union of its children's (initInterior, bvh_accel.dart:518-524) and a leaf's the union of
    // its triangles' vertices (:238-241).  Trees built otherwise keep the v2 kernel.
    for (uint64_t i = 0; ok && i < desc->nnodes; ++i) {
      float lo[3], hi[3];
      if (N[i].nprims == 0) {
        const DrBvhNode &a = N[i + 1], &b = N[N[i].offset];
        for (int k = 0; k < 3; ++k) {
          lo[k] = std::min(a.bmin[k], b.bmin[k]);
          hi[k] = std::max(a.bmax[k], b.bmax[k]);
        }
      } else {
        if ((uint64_t)N[i].offset + N[i].nprims > desc->ntris) return fail(DR_ERR_INVALID, "leaf primitive range");
        for (int k = 0; k < 3; ++k) {
          lo[k] = std::numeric_limits<float>::infinity();
          hi[k] = -lo[k];
        }
        for (uint32_t t = 0; t < N[i].nprims; ++t)
          for (int v = 0; v < 3; ++v) {
            const uint32_t vi = desc->tri_idx[3 * ((uint64_t)N[i].offset + t) + v];
            if (vi >= desc->nverts) return fail(DR_ERR_INVALID, "vertex index out of range");
            for (int k = 0; k < 3; ++k) {
              lo[k] = std::min(lo[k], desc->verts[3 * (size_t)vi + k]);
              hi[k] = std::max(hi[k], desc->verts[3 * (size_t)vi + k]);
            }
          }
      }
      for (int k = 0; k < 3; ++k)
        if (lo[k] != N[i].bmin[k] || hi[k] != N[i].bmax[k]) ok = false;
    }
    if (ok) {
      auto packRef = [&](uint64_t c) -> uint32_t {
        return N[c].nprims ? (PREF_LEAF | ((uint32_t)N[c].nprims << 26) | N[c].offset) : (((uint32_t)N[c].axis << 29) | pairIndex[c]);
      };
      std::vector<DrBvhNode> P(2 * (size_t)std::max<uint32_t>(np, 1));
      for (uint64_t i = 0; i < desc->nnodes; ++i) {
        if (N[i].nprims != 0) continue;
        const uint64_t c[2] = {i + 1, N[i].offset};
        for (int k = 0; k < 2; ++k) {
          DrBvhNode r = N[c[k]];
          if (r.nprims == 0) r.offset = pairIndex[c[k]];
          P[2 * (size_t)pairIndex[i] + k] = r;
        }
      }
      TRY_SC(sc->pairs.alloc(4 * (size_t)std::max<uint32_t>(np, 1)));
      TRY_SC(hipMemcpy(sc->pairs.p, P.data(), P.size() * sizeof(DrBvhNode), hipMemcpyHostToDevice));
      sc->d.pairs = sc->pairs.p;
      sc->d.npairs = np;
      sc->d.rootRef = packRef(0);
    }
  }
  return DR_OK;
}

int SceneBuilder::gatherPrimitives() {
  // primitives: gather vertices on the device
  TRY_SC(sc->tris.alloc(3 * desc->ntris));
  if (desc->ntris) {
    // per-primitive flag byte: bit 0 = Shape.reverseOrientation, bits 1.. = the quadric kind (the device-side validation has
    // checked every index when the host loops did not)
    std::vector<uint8_t> flags(desc->ntris);
    for (uint64_t i = 0; i < desc->ntris; ++i) flags[i] = desc->tri_reverse[i] ? 1 : 0;
    for (uint64_t i = 0; (desc->nquadrics || hostPrep) && i < desc->ntris; ++i) {
      if (desc->tri_idx[3 * i] == DR_PRIM_QUADRIC) {
        const uint32_t qi = desc->tri_idx[3 * i + 1];
        if (qi >= desc->nquadrics) return fail(DR_ERR_INVALID, "quadric index out of range");
        flags[i] |= (uint8_t)(sc->hostQuads[qi].kind << 1);
        sc->hostQuads[qi].reverse = desc->tri_reverse[i] ? 1 : 0;  // Shape.reverseOrientation of the primitive's shape
        continue;
      }
      for (int k = 0; k < 3; ++k)
        if (desc->tri_idx[3 * i + k] >= desc->nverts) return fail(DR_ERR_INVALID, "vertex index out of range");
    }
    for (uint64_t i = 0; hostPrep && i < desc->ntris; ++i) {
      if (desc->tri_material[i] >= desc->nmaterials) return fail(DR_ERR_INVALID, "material index out of range");
      if (desc->tri_light[i] >= (int32_t)desc->nlights) return fail(DR_ERR_INVALID, "light index out of range");
    }
    TRY_SC(hipMemcpy(dR.p, flags.data(), desc->ntris, hipMemcpyHostToDevice));
    launch_gather_tris(dV.p, dI.p, dM.p, dL.p, dR.p, sc->tris.p, desc->ntris, 0);
    TRY_SC(hipDeviceSynchronize());
  }
  return DR_OK;
}

int SceneBuilder::shadingRecords() {
  // per-primitive shading records of meshes with N / S / uv (see ShadeRec in dr_device.h)
  sc->d.srec = nullptr;
  sc->d.xforms = nullptr;
  if (desc->tri_shading && desc->ntris) {
    bool any = false;
    for (uint64_t i = 0; i < desc->ntris; ++i)
      if (desc->tri_shading[i] && desc->tri_idx[3 * i] != DR_PRIM_QUADRIC) any = true;
    if (any) {
      std::vector<float> R(28 * (size_t)desc->ntris, 0.f);
      for (uint64_t i = 0; i < desc->ntris; ++i) {
        const uint32_t f = desc->tri_shading[i];
        if (!f || desc->tri_idx[3 * i] == DR_PRIM_QUADRIC) continue;
        if (f > 7u) return fail(DR_ERR_INVALID, "unknown tri_shading bits");
        if (((f & DR_SHADING_N) && !desc->vert_normals) || ((f & DR_SHADING_S) && !desc->vert_tangents) ||
            ((f & DR_SHADING_UV) && !desc->vert_uvs))
          return fail(DR_ERR_INVALID, "tri_shading names an attribute whose vertex array is missing");
        uint32_t xf = 0;
        if (f & (DR_SHADING_N | DR_SHADING_S)) {
          if (!desc->tri_xform || !desc->mesh_xforms || desc->tri_xform[i] >= desc->nmesh_xforms)
            return fail(DR_ERR_INVALID, "per-vertex normals / tangents need their mesh transform");
          xf = desc->tri_xform[i];
        }
        float* r = &R[28 * (size_t)i];
        for (int k = 0; k < 3; ++k) {
          const size_t v = desc->tri_idx[3 * i + k];
          for (int c = 0; c < 3; ++c) {
            if (f & DR_SHADING_N) r[3 * k + c] = desc->vert_normals[3 * v + c];
            if (f & DR_SHADING_S) r[9 + 3 * k + c] = desc->vert_tangents[3 * v + c];
          }
          if (f & DR_SHADING_UV) {
            r[18 + 2 * k] = desc->vert_uvs[2 * v];
            r[18 + 2 * k + 1] = desc->vert_uvs[2 * v + 1];
          }
        }
        memcpy(&r[24], &f, 4);
        memcpy(&r[25], &xf, 4);
      }
      TRY_SC(sc->srec.alloc(7 * (size_t)desc->ntris));
      TRY_SC(hipMemcpy(sc->srec.p, R.data(), R.size() * sizeof(float), hipMemcpyHostToDevice));
      sc->d.srec = sc->srec.p;
      std::vector<float> X(24 * (size_t)std::max<uint32_t>(desc->nmesh_xforms, 1), 0.f);
      for (uint32_t i = 0; i < desc->nmesh_xforms; ++i)
        for (int k = 0; k < 12; ++k) {
          X[24 * (size_t)i + k] = desc->mesh_xforms[i].object_to_world[k];
          X[24 * (size_t)i + 12 + k] = desc->mesh_xforms[i].world_to_object[k];
        }
      TRY_SC(sc->xforms.alloc(X.size()));
      TRY_SC(hipMemcpy(sc->xforms.p, X.data(), X.size() * sizeof(float), hipMemcpyHostToDevice));
      sc->d.xforms = sc->xforms.p;
    }
  }
  return DR_OK;
}

int SceneBuilder::materials() {
  // materials
  {
    // 4 x float4 per material: (Kd, -) (Kr, type) (Kt, -) (index, sigma: each double's low / high word)
    std::vector<float4> m(4 * (size_t)std::max<uint32_t>(desc->nmaterials, 1), make_float4(0.f, 0.f, 0.f, 0.f));
    auto bitsf = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    for (uint32_t i = 0; i < desc->nmaterials; ++i) {
      const DrMaterial& a = desc->materials[i];
      uint64_t ib, sb;
      memcpy(&ib, &a.index, 8);
      memcpy(&sb, &a.sigma, 8);
      m[4 * i] = make_float4(a.kd[0], a.kd[1], a.kd[2], 0.f);
      m[4 * i + 1] = make_float4(a.kr[0], a.kr[1], a.kr[2], bitsf((uint32_t)a.type));
      m[4 * i + 2] = make_float4(a.kt[0], a.kt[1], a.kt[2], 0.f);
      m[4 * i + 3] = make_float4(bitsf((uint32_t)ib), bitsf((uint32_t)(ib >> 32)), bitsf((uint32_t)sb), bitsf((uint32_t)(sb >> 32)));
    }
    TRY_SC(sc->mats.alloc(m.size()));
    TRY_SC(hipMemcpy(sc->mats.p, m.data(), m.size() * sizeof(float4), hipMemcpyHostToDevice));
  }
  return DR_OK;
}

int SceneBuilder::lights() {
  // lights: ShapeSet areas + Distribution1D (shape_set.dart:40-50; montecarlo.dart:25-52)
  {
    std::vector<DLight> L(std::max<uint32_t>(desc->nlights, 1));
    std::vector<DLightTri> LT(std::max<uint32_t>(desc->nlight_tris, 1));
    std::vector<float> cdf;
    int envLight = -1;
    for (uint32_t i = 0; i < desc->nlights; ++i) {
      const DrAreaLight& a = desc->lights[i];
      if (a.kind == DR_LIGHT_INFINITE) {
        if (a.env_index >= desc->nenv_maps || !desc->env_maps) return fail(DR_ERR_INVALID, "infinite light without a radiance map");
        if (envLight >= 0) return fail(DR_ERR_UNSUPPORTED, "more than one infinite light");
        envLight = (int)i;
        DLight& d = L[i];
        d.L[0] = a.L[0]; d.L[1] = a.L[1]; d.L[2] = a.L[2];
        d.nsamples = std::max(1, a.nsamples);
        d.first_tri = d.ntris = d.cdf_off = 0;
        d.kind = DR_LIGHT_INFINITE;
        d.area = 0.0;
        sc->lightNSamples.push_back(d.nsamples);
        continue;
      }
      if (a.kind == DR_LIGHT_POINT || a.kind == DR_LIGHT_SPOT || a.kind == DR_LIGHT_SPOT_COS || a.kind == DR_LIGHT_DISTANT) {
        DLight& d = L[i];
        memset(&d, 0, sizeof(d));
        d.L[0] = a.L[0]; d.L[1] = a.L[1]; d.L[2] = a.L[2];
        d.nsamples = 1;
        d.kind = a.kind == DR_LIGHT_SPOT_COS ? DR_LIGHT_SPOT : a.kind;
        d.pos[0] = a.position[0]; d.pos[1] = a.position[1]; d.pos[2] = a.position[2];
        if (a.kind == DR_LIGHT_SPOT) {  // spot_light.dart:42-48
          for (int k = 0; k < 12; ++k) d.w2l[k] = a.world_to_light[k];
          d.cosTotalWidth = std::cos((3.141592653589793 / 180.0) * a.cone_width);
          d.cosFalloffStart = std::cos((3.141592653589793 / 180.0) * a.cone_falloff_start);
        } else if (a.kind == DR_LIGHT_SPOT_COS) {  // the cosines a constructed SpotLight keeps (spot_light.dart:46-47)
          for (int k = 0; k < 12; ++k) d.w2l[k] = a.world_to_light[k];
          d.cosTotalWidth = a.cone_width;
          d.cosFalloffStart = a.cone_falloff_start;
        }
        sc->lightNSamples.push_back(1);
        sc->hasDeltaLight = true;
        continue;
      }
      if (a.kind != DR_LIGHT_DIFFUSE_AREA) return fail(DR_ERR_INVALID, "unknown light kind");
      if (a.ntris == 0 || (uint64_t)a.first_tri + a.ntris > desc->nlight_tris) return fail(DR_ERR_INVALID, "light triangle range");
      DLight& d = L[i];
      d.L[0] = a.L[0]; d.L[1] = a.L[1]; d.L[2] = a.L[2];
      d.nsamples = std::max(1, a.nsamples);
      d.first_tri = a.first_tri;
      d.ntris = a.ntris;
      d.kind = DR_LIGHT_DIFFUSE_AREA;
      sc->lightNSamples.push_back(d.nsamples);
      double area = 0.0;
      std::vector<double> areas(a.ntris);
      for (uint32_t t = 0; t < a.ntris; ++t) {
        const DrLightTri& lt = desc->light_tris[a.first_tri + t];
        DLightTri& o = LT[a.first_tri + t];
        if (lt.v[0] == DR_PRIM_QUADRIC) {
          if (lt.v[1] >= desc->nquadrics) return fail(DR_ERR_INVALID, "light quadric index out of range");
          const DQuadric& q = sc->hostQuads[lt.v[1]];
          memset(o.p, 0, sizeof(o.p));
          memcpy(&o.p[0], &lt.v[1], sizeof(uint32_t));
          o.reverse = (lt.reverse_orientation ? 1u : 0u) | ((uint32_t)q.kind << 8);
          if (q.kind == DR_QUADRIC_SPHERE) {
            o.area = q.phiMax * q.radius * (q.zmax - q.zmin);  // sphere.dart:251-253
            for (int k = 0; k < 3; ++k) o.ns[k] = o.nn[k] = 0.f;  // Sphere.sample2 computes Ns per sample
          } else {
            o.area = q.phiMax * 0.5 * (q.radius * q.radius - q.innerRadius * q.innerRadius);  // disk.dart:139-142
            // Ns of Disk.sample (disk.dart:149-153): normalize(objectToWorld.transformNormal((0,0,1))), flipped
            // when reverseOrientation; nn (the hit's dg.nn) depends on the hit point and is evaluated on the device
            double n[3] = {(double)(float)q.w2o[8], (double)(float)q.w2o[9], (double)(float)q.w2o[10]};  // mInv^T * (0,0,1), stored f32
            const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int k = 0; k < 3; ++k) {
              float v = (float)(n[k] / len);
              if (lt.reverse_orientation) v = (float)((double)v * -1.0);
              o.ns[k] = v;
              o.nn[k] = v;
            }
          }
          areas[t] = o.area;
          area += o.area;
          continue;
        }
        for (int k = 0; k < 3; ++k) {
          if (lt.v[k] >= desc->nverts) return fail(DR_ERR_INVALID, "light vertex index out of range");
          for (int c = 0; c < 3; ++c) o.p[3 * k + c] = desc->verts[3 * (size_t)lt.v[k] + c];
        }
        o.reverse = lt.reverse_orientation & 1u;
        o.area = host_tri_area(o.p, o.p + 3, o.p + 6);
        float luv[6];
        const bool hasUV = (lt.reverse_orientation & 2u) != 0;
        if (hasUV) {
          if (!desc->vert_uvs) return fail(DR_ERR_INVALID, "light triangle with uvs but no vert_uvs");
          for (int k = 0; k < 3; ++k) {
            luv[2 * k] = desc->vert_uvs[2 * (size_t)lt.v[k]];
            luv[2 * k + 1] = desc->vert_uvs[2 * (size_t)lt.v[k] + 1];
          }
        }
        host_tri_normals(o.p, o.p + 3, o.p + 6, (lt.reverse_orientation & 1u) != 0, o.nn, o.ns, hasUV ? luv : nullptr);
        areas[t] = o.area;
        area += o.area;
      }
      d.area = area;
      // Distribution1D(areas, n)
      int count = (int)a.ntris;
      std::vector<float> func(count), c(count + 1);
      for (int k = 0; k < count; ++k) func[k] = (float)areas[k];
      c[0] = 0.0f;
      for (int k = 1; k < count + 1; ++k) c[k] = (float)((double)c[k - 1] + (double)func[k - 1] / (double)count);
      double funcInt = c[count];
      if (funcInt == 0.0) {
        for (int k = 1; k < count + 1; ++k) c[k] = (float)((double)k / (double)count);
      } else {
        for (int k = 1; k < count + 1; ++k) c[k] = (float)((double)c[k] / funcInt);
      }
      d.cdf_off = (uint32_t)cdf.size();
      cdf.insert(cdf.end(), c.begin(), c.end());
    }
    if (cdf.empty()) cdf.push_back(0.f);
    memset(&sc->d.env, 0, sizeof(sc->d.env));
    sc->d.hasEnv = 0;
    if (envLight >= 0) {
      const int erc = envLightTables(envLight);
      if (erc) return erc;
    }
    TRY_SC(sc->lights.alloc(L.size()));
    TRY_SC(hipMemcpy(sc->lights.p, L.data(), L.size() * sizeof(DLight), hipMemcpyHostToDevice));
    TRY_SC(sc->ltris.alloc(LT.size()));
    TRY_SC(hipMemcpy(sc->ltris.p, LT.data(), LT.size() * sizeof(DLightTri), hipMemcpyHostToDevice));
    TRY_SC(sc->lcdf.alloc(cdf.size()));
    TRY_SC(hipMemcpy(sc->lcdf.p, cdf.data(), cdf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  return DR_OK;
}

// The InfiniteAreaLight's tables: the radiance map's level 0 (resampled like MIPMap.texture when its size is no power of two) and the
// Distribution2D over luminance x sin(theta) (_setRadianceMap, infinite_area_light.dart:283-307).
int SceneBuilder::envLightTables(int envLight) {
    const DrAreaLight& a = desc->lights[envLight];
    const DrEnvMap& m = desc->env_maps[a.env_index];
    if (!m.texels || m.width <= 0 || m.height <= 0) return fail(DR_ERR_INVALID, "radiance map: null texels or empty size");
    if (m.width > (1 << 14) || m.height > (1 << 14)) return fail(DR_ERR_UNSUPPORTED, "radiance map larger than 16384 texels a side");
    // MIPMap.texture resamples an image whose width or height is no power of two up to the next one (mipmap.dart:71-138) before
    // anything reads it; a host that hands over the decoded image (not a pyramid level) gets the same level 0 here
    std::vector<float> resampled;
    int w = m.width, h = m.height;
    const float* texels = m.texels;
    if ((w & (w - 1)) || (h & (h - 1))) {
      resample_to_pow2(m.texels, w, h, resampled, &w, &h);
      texels = resampled.data();
    }
    // _setRadianceMap (infinite_area_light.dart:283-307): img = luminance(_radiance(u/w, v/h, filter)) * sin(theta),
    // filter = 1/max(w,h).  For a power-of-two map MIPMap.lookup's level = levels-1 + log2(filter) is 0 up to
    // rounding (mipmap.dart:211): either `triangle(0,s,t)` directly or triangle(0)*(1-d) + triangle(1)*d with
    // d ~ 1e-15, which rounds to the same f32 -- so the bilinear level-0 value is used.
    std::vector<float> img((size_t)w * h);
    auto texel = [&](int s, int t, int c) {
      s %= w; if (s < 0) s += w;
      t %= h; if (t < 0) t += h;
      return (double)texels[3 * ((size_t)t * w + s) + c];
    };
    for (int v = 0; v < h; ++v) {
      const double sinTheta = std::sin(3.141592653589793 * (v + 0.5) / h);
      for (int u = 0; u < w; ++u) {
        double s = ((double)u / w) * w - 0.5, t = ((double)v / h) * h - 0.5;
        const int s0 = (int)std::floor(s), t0 = (int)std::floor(t);
        const double ds = s - s0, dt = t - t0;
        double rgbv[3];
        for (int c = 0; c < 3; ++c) {
          double acc = r32(texel(s0, t0, c) * ((1.0 - ds) * (1.0 - dt)));
          acc = r32(acc + r32(texel(s0, t0 + 1, c) * ((1.0 - ds) * dt)));
          acc = r32(acc + r32(texel(s0 + 1, t0, c) * (ds * (1.0 - dt))));
          acc = r32(acc + r32(texel(s0 + 1, t0 + 1, c) * (ds * dt)));
          rgbv[c] = r32(acc * (double)a.L[c]);
        }
        float y = (float)(0.212671 * rgbv[0] + 0.715160 * rgbv[1] + 0.072169 * rgbv[2]);
        img[u + (size_t)v * w] = (float)((double)y * sinTheta);
      }
    }
    // Distribution2D (montecarlo.dart:223-237): one Distribution1D per row + the marginal over their integrals
    auto dist1d = [](const float* f, int count, float* func, float* c, float* funcIntOut) {
      for (int k = 0; k < count; ++k) func[k] = f[k];
      c[0] = 0.0f;
      for (int k = 1; k < count + 1; ++k) c[k] = (float)((double)c[k - 1] + (double)func[k - 1] / (double)count);
      const double funcInt = c[count];
      if (funcInt == 0.0) {
        for (int k = 1; k < count + 1; ++k) c[k] = (float)((double)k / (double)count);
      } else {
        for (int k = 1; k < count + 1; ++k) c[k] = (float)((double)c[k] / funcInt);
      }
      *funcIntOut = (float)funcInt;
    };
    std::vector<float> cf((size_t)w * h), cc((size_t)(w + 1) * h), ci(h), mf(h), mc(h + 1);
    for (int v = 0; v < h; ++v) dist1d(&img[(size_t)v * w], w, &cf[(size_t)v * w], &cc[(size_t)v * (w + 1)], &ci[v]);
    float mi = 0.f;
    dist1d(ci.data(), h, mf.data(), mc.data(), &mi);
    TRY_SC(sc->envTexels.alloc(3 * (size_t)w * h));
    TRY_SC(hipMemcpy(sc->envTexels.p, texels, 3 * (size_t)w * h * sizeof(float), hipMemcpyHostToDevice));
    TRY_SC(sc->envCondFunc.alloc(cf.size()));
    TRY_SC(hipMemcpy(sc->envCondFunc.p, cf.data(), cf.size() * sizeof(float), hipMemcpyHostToDevice));
    TRY_SC(sc->envCondCdf.alloc(cc.size()));
    TRY_SC(hipMemcpy(sc->envCondCdf.p, cc.data(), cc.size() * sizeof(float), hipMemcpyHostToDevice));
    TRY_SC(sc->envCondInt.alloc(ci.size()));
    TRY_SC(hipMemcpy(sc->envCondInt.p, ci.data(), ci.size() * sizeof(float), hipMemcpyHostToDevice));
    TRY_SC(sc->envMargFunc.alloc(mf.size()));
    TRY_SC(hipMemcpy(sc->envMargFunc.p, mf.data(), mf.size() * sizeof(float), hipMemcpyHostToDevice));
    TRY_SC(sc->envMargCdf.alloc(mc.size()));
    TRY_SC(hipMemcpy(sc->envMargCdf.p, mc.data(), mc.size() * sizeof(float), hipMemcpyHostToDevice));
    DEnv& e = sc->d.env;
    // guide rows of the conditional CDFs (DEnv::condGuide): upper_bound at u = k / G, G = w / 4 (a power of two)
    e.condGuide = nullptr;
    e.guideN = 0;
    if (w >= 16 && w + 1 <= 65535) {
      const int G = w / 4;
      std::vector<uint16_t> guide((size_t)h * (G + 1));
      for (int v = 0; v < h; ++v) {
        const float* c = &cc[(size_t)v * (w + 1)];
        int i = 0;  // upper_bound is monotone in u: one sweep per row
        for (int k = 0; k <= G; ++k) {
          const double u = (double)k / (double)G;
          while (i < w + 1 && !(u < (double)c[i])) ++i;
          guide[(size_t)v * (G + 1) + k] = (uint16_t)i;
        }
      }
      TRY_SC(sc->envCondGuide.alloc(guide.size()));
      TRY_SC(hipMemcpy(sc->envCondGuide.p, guide.data(), guide.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      e.condGuide = sc->envCondGuide.p;
      e.guideN = G;
    }
    e.texels = sc->envTexels.p;
    e.condFunc = sc->envCondFunc.p;
    e.condCdf = sc->envCondCdf.p;
    e.condInt = sc->envCondInt.p;
    e.margFunc = sc->envMargFunc.p;
    e.margCdf = sc->envMargCdf.p;
    e.margInt = mi;
    e.w = w;
    e.h = h;
    for (int c = 0; c < 3; ++c) e.L[c] = a.L[c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        e.l2w[3 * r + c] = m.light_to_world[4 * r + c];
        e.w2l[3 * r + c] = m.world_to_light[4 * r + c];
      }
    sc->d.hasEnv = 1;
  return DR_OK;
}

int SceneBuilder::finish() {
  TRY_SC(sc->ctr.alloc(1));
  TRY_SC(hipMemset(sc->ctr.p, 0, sizeof(TraceCounters)));
  TRY_SC(sc->quads.alloc(std::max<size_t>(sc->hostQuads.size(), 1)));
  if (!sc->hostQuads.empty())
    TRY_SC(hipMemcpy(sc->quads.p, sc->hostQuads.data(), sc->hostQuads.size() * sizeof(DQuadric), hipMemcpyHostToDevice));
  sc->d.quads = sc->quads.p;
  sc->d.nquads = (uint32_t)sc->hostQuads.size();
  sc->d.hasSpec = 0;
  for (uint32_t i = 0; i < desc->nmaterials; ++i)
    if (desc->materials[i].type != DR_MATERIAL_MATTE) sc->d.hasSpec = 1;
    else if (desc->materials[i].sigma != 0.0) sc->d.hasSpec = 1;  // Oren-Nayar: general shading kernels too
  if (sc->hasDeltaLight) sc->d.hasSpec = 1;  // point lights are handled by the general kernels
  sc->prtMaterials.clear();  // diffuse PRT names the materials it does not serve (planRender)
  for (uint32_t i = 0; i < desc->nmaterials; ++i)
    sc->prtMaterials.push_back(desc->materials[i].type == DR_MATERIAL_MATTE && desc->materials[i].sigma != 0.0 ? -1 : desc->materials[i].type);
  sc->hasSpecular = false;
  for (uint32_t i = 0; i < desc->nmaterials; ++i)
    if (desc->materials[i].type == DR_MATERIAL_MIRROR || desc->materials[i].type == DR_MATERIAL_GLASS) sc->hasSpecular = true;
  sc->d.nodes = sc->nodes.p;
  sc->d.tris = sc->tris.p;
  sc->d.mats = sc->mats.p;
  sc->d.lights = sc->lights.p;
  sc->d.ltris = sc->ltris.p;
  sc->d.lcdf = sc->lcdf.p;
  sc->d.nnodes = (uint32_t)desc->nnodes;
  // the world bound: node 0's box, whether or not the tree takes the pair layout (diffuse / glossy PRT project the lights at its centre, the
  // probe bake walks inside its bounding sphere and lays its default grid over it); a scene without nodes keeps six zeros
  for (int k = 0; k < 3 && desc->nnodes; ++k) {
    sc->d.rootBox[k] = desc->nodes[0].bmin[k];
    sc->d.rootBox[3 + k] = desc->nodes[0].bmax[k];
  }
  sc->d.ntris = (uint32_t)desc->ntris;
  sc->d.nlights = desc->nlights;
  sc->d.nmats = desc->nmaterials;
  sc->d.nltris = desc->nlight_tris;
  sc->d.ncdf = (uint32_t)sc->lcdf.n;
  // plain triangles + matte materials (the !QUAD shade kernels): the 32-byte shading records (ShTri in dr_device.h)
  sc->d.shtris = nullptr;
  if (!(sc->d.nquads || sc->d.hasSpec || sc->d.srec) && desc->ntris) {
    TRY_SC(sc->shtris.alloc(2 * desc->ntris));
    launch_make_shtris(sc->d, sc->shtris.p, desc->ntris, 0);
    TRY_SC(hipDeviceSynchronize());
    sc->d.shtris = sc->shtris.p;
  }
  return DR_OK;
}

int SceneBuilder::directLightingLayout() {
  {  // DirectLighting: one 1-D + one 2-D slot pair per light for the light sample and one for the BSDF sample, each
     // with roundSize(nSamples) entries (low_discrepancy_sampler.dart:43-49), then the two 1-D volume slots
    auto rp2 = [](int v) { v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v + 1; };
    const size_t nl = sc->lightNSamples.size();
    std::vector<int> ns(nl);
    int n1D = 2;
    for (size_t i = 0; i < nl; ++i) {
      ns[i] = rp2(std::max(1, sc->lightNSamples[i]));
      n1D += 2 * ns[i];
      if (ns[i] != 1) sc->dlMulti = true;
    }
    std::vector<LdBlock> blocks;
    blocks.push_back({0, 1, 1, 0});
    blocks.push_back({2, 1, 1, 0});
    blocks.push_back({4, 1, 0, 0});
    std::vector<DirectStage> stages;
    int o1 = 5, o2 = 5 + n1D;
    for (size_t i = 0; i < nl; ++i) {
      blocks.push_back({o1, ns[i], 0, 0});
      blocks.push_back({o1 + ns[i], ns[i], 0, 0});
      for (int j = 0; j < ns[i]; ++j)
        stages.push_back({(int)i, ns[i], j == ns[i] - 1 ? 1 : 0, o1 + j, o2 + 2 * j, o2 + 2 * ns[i] + 2 * j, o1 + ns[i] + j, 0});
      o1 += 2 * ns[i];
      o2 += 4 * ns[i];
    }
    blocks.push_back({o1, 1, 0, 0});
    blocks.push_back({o1 + 1, 1, 0, 0});
    {  // the 2-D blocks follow all 1-D blocks (montecarlo.dart:441-448)
      int p2 = 5 + n1D;
      for (size_t i = 0; i < nl; ++i) {
        blocks.push_back({p2, ns[i], 1, 0});
        blocks.push_back({p2 + 2 * ns[i], ns[i], 1, 0});
        p2 += 4 * ns[i];
      }
    }
    // strategy "one": ONE EstimateDirect call; light < 0 = "the light floor(u * nLights) of the 1-D slot at float index pad1"; its slots
    // are requested in the order light (1-D, 2-D), lightNum (1-D), BSDF (1-D, 2-D) (direct_lighting_integrator.dart:82-87), then tau / scatter
    stages.push_back({-1, 1, 1, 5, 10, 12, 7, 6});
    sc->dlNBlocks = (int)blocks.size();
    sc->dlNStages = (int)stages.size() - 1;
    sc->dlNFloats = o2;
    sc->dlN1D = n1D;
    TRY_SC(sc->dlBlocks.alloc(blocks.size()));
    TRY_SC(sc->dlStages.alloc(std::max<size_t>(stages.size(), 1)));
    TRY_SC(hipMemcpy(sc->dlBlocks.p, blocks.data(), blocks.size() * sizeof(LdBlock), hipMemcpyHostToDevice));
    if (!stages.empty())
      TRY_SC(hipMemcpy(sc->dlStages.p, stages.data(), stages.size() * sizeof(DirectStage), hipMemcpyHostToDevice));
  }
  return DR_OK;
}
#undef TRY_SC
}  // namespace

extern "C" {

int dr_scene_create(const DrSceneDesc* desc, DrScene** out) {
  if (g_device < 0) return fail(DR_ERR_NO_DEVICE, "dr_init has not been called");
  if (!desc || !out) return fail(DR_ERR_INVALID, "null argument");
  if (desc->ntris > 0 && (!desc->nodes || !desc->verts || !desc->tri_idx || !desc->tri_material || !desc->tri_light ||
                          !desc->tri_reverse || !desc->materials))
    return fail(DR_ERR_INVALID, "scene arrays missing");
  if (desc->ntris >= (1ull << 31) || desc->nnodes >= (1ull << 31)) return fail(DR_ERR_INVALID, "scene too large");
  for (uint32_t i = 0; i < desc->nmaterials; ++i) {
    if (desc->materials[i].type < DR_MATERIAL_MATTE || desc->materials[i].type > DR_MATERIAL_PLASTIC)
      return fail(DR_ERR_INVALID, "unknown material type");
  }
  // k_trace addresses node i at byte offset i * 32 from a scalar base, in 32 bits (dr_trace.hip)
  if (desc->nnodes > (1ull << 27)) return fail(DR_ERR_UNSUPPORTED, "more than 2^27 BVH nodes");
  SceneBuilder B;
  B.desc = desc;
  B.sc = new DrScene();
  memset(&B.sc->stats, 0, sizeof(B.sc->stats));
  // Round 4: validation, height, pair records and the union check run on the device (dr_scene_prep.hip: C4 0.6 s -> 0.1 s).  The
  // serial host loops remain as the reference the device results are tested against (DARTRAY_SCENE_PREP=host).
  B.hostPrep = dr_opt("DARTRAY_SCENE_PREP").is("host");
  int (SceneBuilder::*const steps[])() = {&SceneBuilder::validateOnHost, &SceneBuilder::quadrics, &SceneBuilder::uploadTables, &SceneBuilder::pairsOnDevice,
                                          &SceneBuilder::pairsOnHost, &SceneBuilder::gatherPrimitives, &SceneBuilder::shadingRecords, &SceneBuilder::materials,
                                          &SceneBuilder::lights, &SceneBuilder::finish, &SceneBuilder::directLightingLayout};
  for (auto step : steps) {
    const int rc = (B.*step)();
    if (rc != DR_OK) {
      delete B.sc;
      return rc;
    }
  }
  B.sc->d.traceKernel[0] = B.sc->d.traceKernel[1] = 0;
  B.sc->d.anyFarFirst = 0;
  *out = B.sc;
  return DR_OK;
}

void dr_scene_destroy(DrScene* scene) { delete scene; }

}  // extern "C"
