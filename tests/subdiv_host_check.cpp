// Stand-alone check of the host Loop subdivision builder (dartray_amd/csrc/dr_subdiv_host.cpp) for the host sanitizers: no GPU, no HIP
// runtime, no Python.  Build and run from the repository root:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/subdiv_host_check.cpp dartray_amd/csrc/dr_subdiv_host.cpp -o /tmp/subdiv_host_check && /tmp/subdiv_host_check
// It refines a 6 x 6-vertex grid (50 faces) and an 11-gon bipyramid at nlevels 0 .. 4 into exactly sized buffers (an overrun is the
// sanitizer's to find), checks the counts and that every index is in range, and feeds the builder every input it refuses.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/dartray_hip.h"

static std::string g_error;
int dr_fail(int code, const std::string& msg) {  // the library's is in dr_api.hip
  g_error = msg;
  return code;
}

static int g_failed = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);              \
      ++g_failed;                                                     \
    }                                                                 \
  } while (0)

struct Mesh {
  std::vector<uint32_t> idx;
  std::vector<float> P;
};

static Mesh grid(int n) {
  Mesh m;
  for (int y = 0; y < n; ++y)
    for (int x = 0; x < n; ++x) {
      m.P.push_back((float)x / (n - 1));
      m.P.push_back((float)y / (n - 1));
      m.P.push_back(0.3f * std::sin(1.7f * x + y));
    }
  for (int y = 0; y < n - 1; ++y)
    for (int x = 0; x < n - 1; ++x) {
      const uint32_t a = x + y * n, b = a + 1, c = b + n, d = a + n;
      for (uint32_t v : {a, b, c, a, c, d}) m.idx.push_back(v);
    }
  return m;
}

static Mesh bipyramid(int n) {
  Mesh m;
  for (int i = 0; i < n; ++i) {
    m.P.push_back(std::cos(6.2831853f * i / n));
    m.P.push_back(std::sin(6.2831853f * i / n));
    m.P.push_back(0.1f * std::sin(3.f * i));
  }
  for (float z : {1.f, -0.8f}) {
    m.P.push_back(0.f);
    m.P.push_back(0.f);
    m.P.push_back(z);
  }
  for (int i = 0; i < n; ++i) {
    const uint32_t j = (i + 1) % n;
    for (uint32_t v : {(uint32_t)i, j, (uint32_t)n, j, (uint32_t)i, (uint32_t)n + 1}) m.idx.push_back(v);
  }
  return m;
}

static void refine(const Mesh& m, int nlevels) {
  const uint64_t nf0 = m.idx.size() / 3, nv0 = m.P.size() / 3;
  uint64_t nv = 0, nf = 0;
  CHECK(dr_loop_subdivide(m.idx.data(), nf0, m.P.data(), nv0, nlevels, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == DR_OK);
  CHECK(nf == nf0 << (2 * nlevels));
  std::vector<float> P(3 * nv), N(3 * nv);
  std::vector<uint32_t> idx(3 * nf);
  CHECK(dr_loop_subdivide(m.idx.data(), nf0, m.P.data(), nv0, nlevels, P.data(), N.data(), idx.data(), nv, nf, &nv, &nf) == DR_OK);
  for (uint32_t i : idx) CHECK(i < nv);
  for (float c : P) CHECK(std::isfinite(c));
  for (float c : N) CHECK(std::isfinite(c));
  CHECK(dr_loop_subdivide(m.idx.data(), nf0, m.P.data(), nv0, nlevels, P.data(), N.data(), idx.data(), nv - 1, nf, &nv, &nf) == DR_ERR_INVALID);
}

static void refused(std::vector<uint32_t> idx, uint64_t nverts, int nlevels, int code, const char* what) {
  std::vector<float> P(3 * nverts, 0.25f);
  for (size_t i = 0; i < P.size(); ++i) P[i] += 0.1f * (float)i;
  uint64_t nv = 0, nf = 0;
  g_error.clear();
  CHECK(dr_loop_subdivide(idx.data(), idx.size() / 3, P.data(), nverts, nlevels, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == code);
  if (g_error.find(what) == std::string::npos) {
    std::printf("FAILED: expected \"%s\", got \"%s\"\n", what, g_error.c_str());
    ++g_failed;
  }
}

int main() {
  for (int l = 0; l <= 4; ++l) {
    refine(grid(6), l);
    refine(bipyramid(11), l);
  }
  refused({0, 1, 2}, 4, 1, DR_ERR_INVALID, "a vertex is named by no face");
  refused({0, 1, 5}, 3, 1, DR_ERR_INVALID, "a vertex index is out of range");
  refused({0, 1, 2, 2, 1, 1}, 3, 1, DR_ERR_INVALID, "a face repeats a vertex");
  refused({0, 1, 2, 1, 0, 3, 0, 1, 4}, 5, 1, DR_ERR_INVALID, "an edge is shared by more than two faces");
  refused({0, 1, 2, 0, 1, 3}, 4, 1, DR_ERR_INVALID, "two faces traverse a shared edge in the same direction");
  refused({0, 1, 2, 0, 3, 4}, 5, 1, DR_ERR_INVALID, "the faces of a vertex do not form one fan");
  refused({0, 1, 2}, 3, -1, DR_ERR_INVALID, "nlevels is negative");
  refused({0, 1, 2}, 3, 16, DR_ERR_UNSUPPORTED, "2^31 or more faces or vertices");
  refused({}, 3, 1, DR_ERR_INVALID, "the control mesh is empty");
  std::printf(g_failed ? "subdiv_host_check: %d FAILED\n" : "subdiv_host_check: OK\n", g_failed);
  return g_failed ? 1 : 0;
}
