// Stand-alone check of the host display transform (dartray_amd/csrc/dr_display_host.cpp) for the host sanitizers: no GPU, no HIP runtime,
// no Python.  Build and run from the repository root (tests/test_display.py does):
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tests/display_host_check.cpp dartray_amd/csrc/dr_display_host.cpp -o /tmp/display_host_check && /tmp/display_host_check
// It drives dr_display_host, dr_display_exposure_host and dr_display_table over seeded images of 1 x 1, 1 x 7, 7 x 1, 3 x 2, 17 x 33 and
// 64 x 64 pixels, sprinkled with NaN, infinities, negatives, zeros, subnormals and values up to 3e38, for every curve, encode and exposure
// mode, out of and into exactly sized heap buffers (an overrun is the sanitizer's to find; a float-to-integer conversion out of range the
// undefined-behaviour sanitizer's), checks what must hold of any output, and feeds the entry points every input they refuse.
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

static uint32_t g_state = 4321u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) / 16777216.0f;
}

static const uint32_t kInvalid = 0x80FF10C0u;

static void transform(int w, int h, uint32_t curve, uint32_t encode, uint32_t automatic, int kind) {
  const size_t n = (size_t)w * h;
  std::vector<float> rgb(3 * n);
  std::vector<uint8_t> out(4 * n, 7);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float special[12] = {nan, inf, -inf, -1.0f, 0.0f, -0.0f, 1e-45f, 1e-39f, 1.17549435e-38f, 1e30f, 3e38f, -3e38f};
  for (size_t p = 0; p < n; ++p) {
    for (int c = 0; c < 3; ++c) rgb[3 * p + c] = kind == 1 ? 0.42f : kind == 2 ? nan : std::exp(14.0f * rnd() - 9.0f);
    if (kind == 0 && rnd() < 0.3f) rgb[3 * p + (p % 3)] = special[(p / 3) % 12];
  }
  const DrDisplayParams prm{curve, encode, automatic, (uint32_t)(1000.0f * rnd()), 0.05f + 4.0f * rnd(), 0.18f, rnd() < 0.5f ? 0.0f : 0.25f, kInvalid};
  CHECK(dr_display_host(rgb.data(), w, h, &prm, out.data()) == DR_OK);
  std::vector<uint32_t> hist(DR_DISPLAY_BINS, 7u);
  float scale = -1.0f;
  CHECK(dr_display_exposure_host(rgb.data(), w, h, &prm, &scale, hist.data()) == DR_OK);
  uint64_t counted = 0, valid = 0;
  for (uint32_t b = 0; b < DR_DISPLAY_BINS; ++b) counted += hist[b];
  for (uint32_t b = 0; b < 8; ++b) CHECK(hist[b] == 0 && hist[DR_DISPLAY_BINS - 1 - b] == 0);  // subnormals and infinities are not counted
  for (size_t p = 0; p < n; ++p) {
    const bool ok = std::isfinite(rgb[3 * p]) && std::isfinite(rgb[3 * p + 1]) && std::isfinite(rgb[3 * p + 2]);
    valid += ok;
    uint32_t px;
    std::memcpy(&px, &out[4 * p], 4);
    if (ok) CHECK(out[4 * p + 3] == 255);
    else CHECK(px == kInvalid);
  }
  CHECK(counted <= valid);
  CHECK(counted == 0 ? scale == 1.0f : (scale > 0.0f));
  float again = -1.0f;
  CHECK(dr_display_exposure_host(rgb.data(), w, h, &prm, &again, nullptr) == DR_OK && std::memcmp(&again, &scale, 4) == 0);
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
  const int sizes[6][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 2}, {17, 33}, {64, 64}};
  for (const auto& s : sizes)
    for (uint32_t curve = 0; curve < 3; ++curve)
      for (uint32_t encode = 0; encode < 3; ++encode)
        for (uint32_t automatic = 0; automatic < 2; ++automatic)
          for (int kind = 0; kind < 3; ++kind) transform(s[0], s[1], curve, encode, automatic, kind);
  // the tables, into exactly sized buffers
  for (uint32_t encode = 0; encode < 3; ++encode) {
    std::vector<uint32_t> t(256, 7u);
    CHECK(dr_display_table(encode, t.data(), 256) == DR_OK);
    if (encode == DR_ENCODE_REFERENCE) {
      CHECK(t[0] == 0 && t[255] == 255);
      for (int i = 1; i < 256; ++i) CHECK(t[i] >= t[i - 1] && t[i] <= 255);
    } else {
      CHECK(t[0] == 0);
      for (int i = 2; i < 256; ++i) CHECK(t[i] > t[i - 1]);  // positive floats order as their bits do
    }
  }
  std::vector<uint32_t> t(256);
  refused(dr_display_table(3, t.data(), 256), "encode must be");
  refused(dr_display_table(0, nullptr, 256), "a null pointer");
  refused(dr_display_table(0, t.data(), 255), "n must be 256");
  std::vector<float> a(3 * 6);
  std::vector<uint8_t> o(4 * 6);
  const DrDisplayParams ok{DR_TONE_REINHARD, DR_ENCODE_SRGB, 1, 500, 1.0f, 0.18f, 0.0f, 0xff000000u};
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  float scale = 0.0f;
  refused(dr_display_host(nullptr, 3, 2, &ok, o.data()), "a null pointer");
  refused(dr_display_host(a.data(), 3, 2, nullptr, o.data()), "a null pointer");
  refused(dr_display_host(a.data(), 3, 2, &ok, nullptr), "a null pointer");
  refused(dr_display_exposure_host(a.data(), 3, 2, &ok, nullptr, nullptr), "a null pointer");
  refused(dr_display_exposure_host(nullptr, 3, 2, &ok, &scale, nullptr), "a null pointer");
  refused(dr_display_check(nullptr, 3, 2), "a null pointer");
  refused(dr_display_host(a.data(), 0, 2, &ok, o.data()), "w and h must be at least 1");
  refused(dr_display_host(a.data(), 3, -1, &ok, o.data()), "w and h must be at least 1");
  refused(dr_display_host(a.data(), 65536, 32768, &ok, o.data()), "2^31 or more pixels");
  refused(dr_display_host(a.data(), 3, 2, &ok, (uint8_t*)a.data() + 71), "out overlaps an input");
  DrDisplayParams p = ok;
  p.curve = 3;
  refused(dr_display_check(&p, 3, 2), "curve must be");
  p = ok;
  p.encode = 7;
  refused(dr_display_host(a.data(), 3, 2, &p, o.data()), "encode must be");
  p = ok;
  p.permille = 1001;
  refused(dr_display_check(&p, 3, 2), "permille must be in 0..1000");
  for (float bad : {0.0f, -1.0f, inf, nan}) {
    p = ok;
    p.exposure = bad;
    refused(dr_display_check(&p, 3, 2), "exposure must be finite and positive");
    p = ok;
    p.key = bad;
    refused(dr_display_exposure_host(a.data(), 3, 2, &p, &scale, nullptr), "key must be finite and positive");
  }
  for (float bad : {-1.0f, inf, nan}) {
    p = ok;
    p.inv_white2 = bad;
    refused(dr_display_check(&p, 3, 2), "inv_white2 must be finite and not negative");
  }
  CHECK(dr_display_check(&ok, 3, 2) == DR_OK);
  std::printf(g_failed ? "display_host_check: %d FAILED\n" : "display_host_check: OK\n", g_failed);
  return g_failed ? 1 : 0;
}
