// Stand-alone check of the host firefly clamp (dartray_amd/csrc/dr_firefly_host.cpp) for the host sanitizers: no GPU, no HIP runtime, no
// Python.  Build and run from the repository root (tests/test_firefly.py does):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tests/firefly_host_check.cpp dartray_amd/csrc/dr_firefly_host.cpp -o /tmp/firefly_host_check && /tmp/firefly_host_check
// It drives dr_firefly_host over seeded images of 1 x 1, 1 x 7, 7 x 1, 5 x 7, 65 x 5 and 64 x 48 pixels, sprinkled with NaN, infinities,
// negatives, zeros of both signs, subnormals and values up to the largest f32 in every plane, for every radius and rank and three limits,
// with and without the removed plane, out of and into exactly sized heap buffers (a tap outside the image is the sanitizer's to find),
// checks what must hold of any output, and feeds the entry points every input they refuse.
#include <cmath>
#include <cstdio>
#include <cstring>
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

static uint32_t g_state = 9876u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) / 16777216.0f;
}

static float lum(const float* c) { return (0.212671f * c[0] + 0.715160f * c[1]) + 0.072169f * c[2]; }

static long g_clamped = 0, g_kept = 0;

static void clamp(int w, int h, int kind, const DrFireflyParams& prm, bool with_removed) {
  const size_t n = (size_t)w * h;
  std::vector<float> rgb(3 * n), normal(3 * n), depth(n), out(3 * n, -7.0f), removed(with_removed ? n : 0, -7.0f);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float special[12] = {nan, inf, -inf, -1.0f, 0.0f, -0.0f, 1e-45f, 1e-39f, 1.17549435e-38f, 1e30f, 3.4028235e38f, -3e38f};
  for (size_t p = 0; p < n; ++p) {
    const float level = kind == 1 ? 0.42f : std::exp(10.0f * rnd() - 6.0f);
    for (int c = 0; c < 3; ++c) {
      rgb[3 * p + c] = level * (rnd() < 0.05f ? 80.0f : 1.0f);
      normal[3 * p + c] = 0.5f + (p % 7 < 5 ? 0.0f : 0.3f) + 0.01f * rnd();
    }
    depth[p] = (p % 5 < 4 ? 3.0f : 7.0f) + 0.01f * rnd();
    if (kind == 0 && rnd() < 0.3f) {
      const float v = special[(p / 3) % 12];
      const float pick = rnd();
      if (pick < 0.6f) rgb[3 * p + (p % 3)] = v;
      else if (pick < 0.8f) normal[3 * p + (p % 3)] = v;
      else depth[p] = v;
    }
  }
  CHECK(dr_firefly_host(rgb.data(), normal.data(), depth.data(), w, h, &prm, out.data(), with_removed ? removed.data() : nullptr) == DR_OK);
  for (size_t p = 0; p < n; ++p) {
    const bool same = std::memcmp(&out[3 * p], &rgb[3 * p], 12) == 0;
    bool valid = std::isfinite(depth[p]) && std::isfinite(lum(&rgb[3 * p]));
    for (int c = 0; c < 3; ++c) valid = valid && std::isfinite(rgb[3 * p + c]) && std::isfinite(normal[3 * p + c]);
    if (!valid) CHECK(same);
    if (with_removed) {
      CHECK(removed[p] >= 0.0f);
      CHECK((removed[p] == 0.0f) == same);
    }
    if (!same) {
      CHECK(lum(&out[3 * p]) < lum(&rgb[3 * p]));
      for (int c = 0; c < 3; ++c) CHECK(std::fabs(out[3 * p + c]) <= std::fabs(rgb[3 * p + c]));
    }
    g_clamped += !same;
    g_kept += same && valid;
  }
}

static void refused(int rc, const char* what) {
  CHECK(rc == DR_ERR_INVALID);
  if (g_error.find(what) == std::string::npos) {
    std::printf("FAILED: expected \"%s\", got \"%s\"\n", what, g_error.c_str());
    ++g_failed;
  }
  g_error.clear();
}

int main() {
  const int sizes[6][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 7}, {65, 5}, {64, 48}};
  const float limits[3][2] = {{4.0f, 0.0f}, {0.0f, 0.0f}, {1.5f, 0.25f}};
  for (const auto& s : sizes)
    for (int radius = 1; radius <= 2; ++radius)
      for (int rank = 1; rank <= 4; ++rank)
        for (const auto& l : limits)
          for (int kind = 0; kind < 2; ++kind) {
            const DrFireflyParams prm{radius, rank, l[0], l[1], 0.02f, 0.05f};
            clamp(s[0], s[1], kind, prm, (radius + rank + kind) % 2 == 0);
          }
  CHECK(g_clamped > 1000 && g_kept > 1000);
  std::vector<float> a(3 * 6), nrm(3 * 6), z(6), o(3 * 6 + 6);
  const DrFireflyParams ok{1, 2, 4.0f, 0.0f, 0.02f, 0.05f};
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  float* rem = o.data() + 18;
  refused(dr_firefly_host(nullptr, nrm.data(), z.data(), 3, 2, &ok, o.data(), rem), "a null pointer");
  refused(dr_firefly_host(a.data(), nullptr, z.data(), 3, 2, &ok, o.data(), rem), "a null pointer");
  refused(dr_firefly_host(a.data(), nrm.data(), nullptr, 3, 2, &ok, o.data(), rem), "a null pointer");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, 2, nullptr, o.data(), rem), "a null pointer");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, 2, &ok, nullptr, rem), "a null pointer");
  refused(dr_firefly_check(nullptr, 3, 2), "a null pointer");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 0, 2, &ok, o.data(), rem), "w and h must be at least 1");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, -1, &ok, o.data(), rem), "w and h must be at least 1");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 65536, 32768, &ok, o.data(), rem), "2^31 or more pixels");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, 2, &ok, a.data() + 17, rem), "an output overlaps an input");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, 2, &ok, o.data(), z.data() + 5), "an output overlaps an input");
  refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, 2, &ok, o.data(), o.data() + 17), "an output overlaps another output");
  DrFireflyParams p = ok;
  for (int bad : {0, 3, -1}) {
    p = ok;
    p.radius = bad;
    refused(dr_firefly_check(&p, 3, 2), "radius must be 1 or 2");
  }
  for (int bad : {0, 5, -1}) {
    p = ok;
    p.rank = bad;
    refused(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, 2, &p, o.data(), rem), "rank must be in 1..4");
  }
  for (float bad : {-1.0f, inf, -inf, nan}) {
    p = ok;
    p.threshold = bad;
    refused(dr_firefly_check(&p, 3, 2), "threshold must be finite and not negative");
    p = ok;
    p.floor = bad;
    refused(dr_firefly_check(&p, 3, 2), "floor must be finite and not negative");
    p = ok;
    p.depth_tol = bad;
    refused(dr_firefly_check(&p, 3, 2), "depth_tol and normal_tol must be finite and not negative");
    p = ok;
    p.normal_tol = bad;
    refused(dr_firefly_check(&p, 3, 2), "depth_tol and normal_tol must be finite and not negative");
  }
  CHECK(dr_firefly_check(&ok, 3, 2) == DR_OK);
  CHECK(dr_firefly_host(a.data(), nrm.data(), z.data(), 3, 2, &ok, o.data(), nullptr) == DR_OK);
  std::printf(g_failed ? "firefly_host_check: %d FAILED\n" : "firefly_host_check: OK\n", g_failed);
  return g_failed ? 1 : 0;
}
