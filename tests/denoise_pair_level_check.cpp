// One level of the variance-guided a-trous filter (dr_denoise_pair.h's dnp_pixel) over planes given as they are: the
// entry points pack their planes themselves, and no packed plane lets a level take a pixel's validity away (2.19, "Validity"), so
// tests/test_denoise_pair.py hands that rule planes no pack produces.
//   denoise_pair_level_check IN OUT     IN: int32 w, h, s; f32 k_color, k_normal, k_depth, var_floor; colour[h][w][4]; guide[h][w][4]
//                                       OUT: colour[h][w][4] of the level
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../dartray_amd/csrc/dr_denoise_pair.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t whs[3];
  float k[4];
  if (fread(whs, sizeof(int32_t), 3, in) != 3 || fread(k, sizeof(float), 4, in) != 4 || whs[0] < 1 || whs[1] < 1 || whs[0] > 4096 || whs[1] > 4096) return 4;
  const int32_t w = whs[0], h = whs[1];
  const size_t n = (size_t)w * (size_t)h;
  std::vector<DnTexel> colour(n), guide(n), out(n);
  if (fread(colour.data(), sizeof(DnTexel), n, in) != n || fread(guide.data(), sizeof(DnTexel), n, in) != n) return 5;
  fclose(in);
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) out[(size_t)y * w + x] = dnp_pixel(colour.data(), guide.data(), w, h, x, y, whs[2], k[0], k[1], k[2], k[3]);
  FILE* o = fopen(argv[2], "wb");
  if (!o || fwrite(out.data(), sizeof(DnTexel), n, o) != n || fclose(o) != 0) return 6;
  printf("denoise_pair_level_check: OK\n");
  return 0;
}
