// Stand-alone check of the host a-trous filter (dartray_amd/csrc/dr_denoise_host.cpp) for the host sanitizers: no GPU, no HIP runtime,
// no Python.  Build and run from the repository root (tests/test_denoise.py does):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tests/denoise_host_check.cpp dartray_amd/csrc/dr_denoise_host.cpp -o /tmp/denoise_host_check && /tmp/denoise_host_check
// It filters seeded images of 1 x 1, 1 x 7, 7 x 1, 3 x 2, 17 x 33 and 64 x 64 pixels, sprinkled with non-finite values, at 1, 2, 5 and 8
// levels (step 128 at the last: every tap but the centre's lies outside) out of and into exactly sized heap buffers (an overrun is the
// sanitizer's to find), checks that a constant image comes back as it is and that non-valid pixels pass through, and feeds the entry
// point every input it refuses.
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

static uint32_t g_state = 12345u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) / 16777216.0f;
}

static void filter(int w, int h, int iterations, bool constant) {
  const size_t n = (size_t)w * h;
  std::vector<float> rgb(3 * n), normal(3 * n), depth(n), out(3 * n, -1.0f);
  const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
  for (size_t p = 0; p < n; ++p) {
    for (int c = 0; c < 3; ++c) {
      rgb[3 * p + c] = constant ? 0.5f : 4.0f * rnd();
      normal[3 * p + c] = constant ? 0.25f : rnd();
    }
    depth[p] = constant ? 3.0f : 20.0f + 10.0f * rnd();
    if (!constant && rnd() < 0.05f) rgb[3 * p + (p % 3)] = bad[p % 3];
    if (!constant && rnd() < 0.05f) (p % 2 ? depth[p] : normal[3 * p + 1]) = bad[(p + 1) % 3];
  }
  const DrDenoiseParams prm{iterations, 1.0f, 100.0f, 0.5f};
  CHECK(dr_denoise_atrous_host(rgb.data(), normal.data(), depth.data(), w, h, &prm, out.data()) == DR_OK);
  for (size_t p = 0; p < n; ++p) {
    bool valid = std::isfinite(depth[p]);
    for (int c = 0; c < 3; ++c) valid = valid && std::isfinite(rgb[3 * p + c]) && std::isfinite(normal[3 * p + c]);
    if (constant || !valid) {
      CHECK(std::memcmp(&out[3 * p], &rgb[3 * p], 3 * sizeof(float)) == 0);
    } else {
      for (int c = 0; c < 3; ++c) CHECK(out[3 * p + c] >= 0.0f && out[3 * p + c] <= 4.001f);  // a convex combination of valid colours, rounded
    }
  }
}

static void refused(const float* rgb, const float* normal, const float* depth, int w, int h, const DrDenoiseParams* prm, float* out,
                    const char* what) {
  g_error.clear();
  CHECK(dr_denoise_atrous_host(rgb, normal, depth, w, h, prm, out) == DR_ERR_INVALID);
  if (g_error.find(what) == std::string::npos) {
    std::printf("FAILED: expected \"%s\", got \"%s\"\n", what, g_error.c_str());
    ++g_failed;
  }
}

int main() {
  const int sizes[6][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 2}, {17, 33}, {64, 64}};
  for (const auto& s : sizes)
    for (int it : {1, 2, 5, 8}) {
      filter(s[0], s[1], it, false);
      filter(s[0], s[1], it, true);
    }
  std::vector<float> a(3 * 6), b(3 * 6), d(6), o(3 * 6);
  const DrDenoiseParams ok{2, 1.0f, 1.0f, 1.0f};
  const float inf = std::numeric_limits<float>::infinity();
  refused(nullptr, b.data(), d.data(), 3, 2, &ok, o.data(), "a null pointer");
  refused(a.data(), b.data(), d.data(), 3, 2, nullptr, o.data(), "a null pointer");
  refused(a.data(), b.data(), d.data(), 3, 2, &ok, nullptr, "a null pointer");
  refused(a.data(), b.data(), d.data(), 0, 2, &ok, o.data(), "w and h must be at least 1");
  refused(a.data(), b.data(), d.data(), 3, -1, &ok, o.data(), "w and h must be at least 1");
  refused(a.data(), b.data(), d.data(), 65536, 32768, &ok, o.data(), "2^31 or more pixels");
  for (int it : {0, 9, -3}) {
    const DrDenoiseParams p{it, 1.0f, 1.0f, 1.0f};
    refused(a.data(), b.data(), d.data(), 3, 2, &p, o.data(), "iterations must be in 1..8");
  }
  for (float k : {-1.0f, inf, std::numeric_limits<float>::quiet_NaN()})
    for (int which = 0; which < 3; ++which) {
      DrDenoiseParams p = ok;
      (which == 0 ? p.k_color : which == 1 ? p.k_normal : p.k_depth) = k;
      refused(a.data(), b.data(), d.data(), 3, 2, &p, o.data(), "must be finite and not negative");
    }
  const DrDenoiseParams big{2, 3.0e38f, 1.0f, 1.0f};
  refused(a.data(), b.data(), d.data(), 3, 2, &big, o.data(), "k_color of the last level is not finite");
  refused(a.data(), b.data(), d.data(), 3, 2, &ok, a.data(), "out overlaps an input");
  refused(a.data(), b.data(), d.data(), 3, 1, &ok, b.data() + 8, "out overlaps an input");
  refused(a.data(), b.data(), o.data() + 17, 3, 2, &ok, o.data(), "out overlaps an input");
  std::printf(g_failed ? "denoise_host_check: %d FAILED\n" : "denoise_host_check: OK\n", g_failed);
  return g_failed ? 1 : 0;
}
