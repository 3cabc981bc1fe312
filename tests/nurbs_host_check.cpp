// Stand-alone check of the host NURBS builder (dartray_amd/csrc/dr_nurbs_host.cpp) for the host sanitizers: no GPU, no HIP runtime, no
// Python.  Build and run from the repository root (tests/test_nurbs.py does):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tests/nurbs_host_check.cpp dartray_amd/csrc/dr_nurbs_host.cpp -o /tmp/nurbs_host_check && /tmp/nurbs_host_check
// It dices patches of every order 2 .. 8 (single span and several spans, 'P' and 'Pw', whole range and sub-range, the
// order-8 patch at both ends of its knot range) at 30 x 30, 2 x 2, 65 x 3 and 3 x 257 out of and into exactly sized heap buffers -- an
// overrun is the sanitizer's to find --, checks what must hold of any output, and feeds the entry point every input it refuses.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../include/dartray_hip.h"

static std::string g_error;
int dr_fail(int code, const std::string& msg) {  // the library's is in dr_api.hip
  g_error = msg;
  return code;
}

static int g_failed = 0;
#define CHECK(c)                                         \
  do {                                                   \
    if (!(c)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #c); \
      ++g_failed;                                        \
    }                                                    \
  } while (0)

static uint32_t g_state = 97531u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) / 16777216.0f;
}

struct Patch {
  std::vector<float> uk, vk, cp;  // exactly sized
  DrNurbsPatch d;
};

// order x order, n = order + extra control points per direction, knots 0 (order times), 1, 2 .. extra, extra + 1 (order times)
static Patch make(int uorder, int vorder, int uextra, int vextra, bool homogeneous) {
  Patch p;
  auto knots = [](int order, int extra) {
    std::vector<float> k;
    for (int i = 0; i < order; ++i) k.push_back(0.0f);
    for (int i = 1; i <= extra; ++i) k.push_back((float)i);
    for (int i = 0; i < order; ++i) k.push_back((float)(extra + 1));
    return k;
  };
  p.uk = knots(uorder, uextra);
  p.vk = knots(vorder, vextra);
  const int nu = uorder + uextra, nv = vorder + vextra;
  for (int j = 0; j < nv; ++j)
    for (int i = 0; i < nu; ++i) {
      const float w = homogeneous ? 0.5f + rnd() : 1.0f;
      p.cp.push_back((float)i * w);
      p.cp.push_back((float)j * w);
      p.cp.push_back((rnd() - 0.5f) * w);
      if (homogeneous) p.cp.push_back(w);
    }
  p.d = DrNurbsPatch{nu, uorder, p.uk.data(), 0.0f, (float)(uextra + 1), nv, vorder, p.vk.data(), 0.0f, (float)(vextra + 1), p.cp.data(), homogeneous ? 1 : 0, 0, 0, 0};
  return p;
}

static void run(const DrNurbsPatch& d, bool expect_finite_P) {
  uint64_t nverts = 0, ntris = 0;
  CHECK(dr_nurbs_dice(&d, nullptr, nullptr, nullptr, nullptr, 0, 0, &nverts, &ntris) == DR_OK);
  const uint32_t du = d.diceu ? d.diceu : 30u, dv = d.dicev ? d.dicev : 30u;
  CHECK(nverts == (uint64_t)du * dv && ntris == 2ull * (du - 1) * (dv - 1));
  std::vector<float> P(3 * nverts), N(3 * nverts), uv(2 * nverts);
  std::vector<uint32_t> idx(3 * ntris);
  CHECK(dr_nurbs_dice(&d, P.data(), N.data(), uv.data(), idx.data(), nverts, ntris, nullptr, nullptr) == DR_OK);
  for (uint32_t i : idx) CHECK(i < nverts);
  CHECK(uv[0] == d.u0 && uv[1] == d.v0 && uv[2 * nverts - 2] == d.u1 && uv[2 * nverts - 1] == d.v1);
  if (expect_finite_P)
    for (float x : P) CHECK(std::isfinite(x));
  if (nverts > 1) {  // one vertex short: refused, nothing written
    std::vector<float> P2(3 * (nverts - 1), 7.0f);
    CHECK(dr_nurbs_dice(&d, P2.data(), N.data(), uv.data(), idx.data(), nverts - 1, ntris, nullptr, nullptr) == DR_ERR_INVALID);
    for (float x : P2) CHECK(x == 7.0f);
  }
}

static void refuse(DrNurbsPatch d, const char* needle) {
  uint64_t nverts = 7, ntris = 7;
  g_error.clear();
  CHECK(dr_nurbs_dice(&d, nullptr, nullptr, nullptr, nullptr, 0, 0, &nverts, &ntris) == DR_ERR_INVALID);
  if (g_error.find(needle) == std::string::npos) {
    std::printf("FAILED: expected \"%s\" in \"%s\"\n", needle, g_error.c_str());
    ++g_failed;
  }
  CHECK(nverts == 7 && ntris == 7);
}

int main() {
  const uint32_t rates[4][2] = {{0, 0}, {2, 2}, {65, 3}, {3, 257}};
  for (int order = 2; order <= DR_NURBS_MAX_ORDER; ++order)
    for (int extra = 0; extra <= 2; extra += 2)
      for (int homogeneous = 0; homogeneous <= 1; ++homogeneous) {
        Patch p = make(order, order == 2 ? 2 : order - 1, extra, extra ? 1 : 0, homogeneous != 0);
        for (const auto& r : rates) {
          p.d.diceu = r[0];
          p.d.dicev = r[1];
          run(p.d, true);
        }
        p.d.u0 = 0.25f;
        p.d.u1 = 0.75f;
        p.d.v0 = 0.875f;
        p.d.v1 = 0.125f;  // a range may run backwards
        run(p.d, true);
      }
  {  // order 8 at both ends of the knot range: every dice point on the first, then on the last knot
    Patch p = make(8, 8, 0, 0, true);
    p.d.diceu = p.d.dicev = 3;
    p.d.u0 = p.d.u1 = p.d.v0 = p.d.v1 = 0.0f;
    run(p.d, true);
    p.d.u0 = p.d.u1 = p.d.v0 = p.d.v1 = 1.0f;
    run(p.d, true);
    Patch q = make(8, 8, 3, 3, false);  // ... and of a knot range of four spans
    q.d.diceu = q.d.dicev = 3;
    q.d.u0 = q.d.u1 = q.d.v0 = q.d.v1 = 4.0f;
    run(q.d, true);
  }
  {  // computed, not repaired: a zero knot span (every knot equal) and a zero weight
    Patch p = make(3, 3, 0, 0, true);
    for (float& k : p.uk) k = 0.5f;
    p.d.u0 = p.d.u1 = 0.5f;
    run(p.d, false);
    Patch q = make(3, 3, 0, 0, true);
    for (size_t i = 3; i < q.cp.size(); i += 4) q.cp[i] = 0.0f;
    run(q.d, false);
  }

  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  Patch b = make(4, 4, 2, 2, false);
  uint64_t nverts = 0, ntris = 0;
  CHECK(dr_nurbs_dice(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, &nverts, &ntris) == DR_ERR_INVALID);
  DrNurbsPatch d = b.d;
  d.uorder = 1, refuse(d, "uorder is below 2 or above DR_NURBS_MAX_ORDER");
  d = b.d, d.vorder = 9, refuse(d, "vorder is below 2 or above DR_NURBS_MAX_ORDER");
  d = b.d, d.nu = 3, refuse(d, "nu is below uorder");
  d = b.d, d.nv = -5, refuse(d, "nv is below vorder");
  d = b.d, d.uknots = nullptr, refuse(d, "uknots is null");
  d = b.d, d.vknots = nullptr, refuse(d, "vknots is null");
  d = b.d, d.cp = nullptr, refuse(d, "cp is null");
  d = b.d, d.u0 = -0.5f, refuse(d, "u0 or u1 is outside");
  d = b.d, d.u1 = 3.5f, refuse(d, "u0 or u1 is outside");
  d = b.d, d.v0 = nan, refuse(d, "v0 or v1 is outside");
  d = b.d, d.v1 = inf, refuse(d, "v0 or v1 is outside");
  d = b.d, d.diceu = 1, refuse(d, "diceu or dicev is below 2 or above 4096");
  d = b.d, d.dicev = 4097, refuse(d, "diceu or dicev is below 2 or above 4096");
  d = b.d, d.diceu = 4096, d.dicev = 2048, refuse(d, "diceu * dicev is above 2^22");
  {
    Patch k = make(4, 4, 2, 2, false);
    k.uk[5] = 0.5f;  // 0 0 0 0 1 0.5 3 ...
    refuse(k.d, "the u knot vector decreases");
    Patch n = make(4, 4, 2, 2, false);
    n.vk[9] = nan;
    refuse(n.d, "a v knot is not finite");
    n.vk[9] = inf;
    refuse(n.d, "a v knot is not finite");
  }
  std::vector<float> P(2700), N(2700), uv(1800);
  CHECK(dr_nurbs_dice(&b.d, P.data(), N.data(), uv.data(), nullptr, 900, 1682, nullptr, nullptr) == DR_ERR_INVALID);

  if (g_failed) {
    std::printf("nurbs_host_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("nurbs_host_check: OK\n");
  return 0;
}
