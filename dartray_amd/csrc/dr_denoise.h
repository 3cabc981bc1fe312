// dr_denoise.h -- the edge-avoiding a-trous filter (Dammertz et al. 2010 with rational edge-stopping weights; the
// reference has no denoiser): the packed planes, the tap table, one pixel's share of a level and the parameter check, written once
// for the host loop (dr_denoise_host.cpp) and the device kernels (dr_denoise_device.hip).
//
// A level reads two planes of 16-byte texels, colour = (r, g, b, valid) and guide = (nx, ny, nz, z), and gives every pixel its new
// colour.  `valid` is 1 where the pixel's three colour values (those of this level's input), its three normal values and its depth
// are all finite, else 0; the guides never change, so a level's output keeps a pixel valid exactly while its new colour is finite.
//
// Arithmetic: + - * / in f32, one operation and one rounding per operator, in the order DESIGN.md 2.15 writes them; the units that
// include this header are compiled with -ffp-contract=off and without fast-math, and `/` is the correctly rounded division.
#ifndef DR_DENOISE_H
#define DR_DENOISE_H

#include <utility>
#include <vector>

#include "dr_image.h"

#define DR_DN_MAX_ITERATIONS 8

// h[a] * h[b] of h = [1/16, 1/4, 3/8, 1/4, 1/16], row dy + 2, column dx + 2: multiples of 1/256, exact in f32
DR_DN_HD float dn_tap(int row, int col) {
  static constexpr float H[5][5] = {{1 / 256.f, 4 / 256.f, 6 / 256.f, 4 / 256.f, 1 / 256.f},
                                    {4 / 256.f, 16 / 256.f, 24 / 256.f, 16 / 256.f, 4 / 256.f},
                                    {6 / 256.f, 24 / 256.f, 36 / 256.f, 24 / 256.f, 6 / 256.f},
                                    {4 / 256.f, 16 / 256.f, 24 / 256.f, 16 / 256.f, 4 / 256.f},
                                    {1 / 256.f, 4 / 256.f, 6 / 256.f, 4 / 256.f, 1 / 256.f}};
  return H[row][col];
}

// One pixel of one level: step s, sharpness kc (this level's), kn, kz.  Every tap's coordinates are checked against the image
// before its two loads (64-bit: x + 2 * 128 may leave the range of an int in an image 2^31 - 1 pixels wide).
DR_DN_HD DnTexel dn_pixel(const DnTexel* colour, const DnTexel* guide, int32_t w, int32_t h, int32_t x, int32_t y, int32_t s, float kc,
                          float kn, float kz) {
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const DnTexel cp = colour[p];
  if (cp.w == 0.0f) return cp;  // not valid: the input colour, bit for bit
  const DnTexel gp = guide[p];
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sumw = 0.0f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = (int64_t)y + (int64_t)dy * s;
    if (qy < 0 || qy >= h) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = (int64_t)x + (int64_t)dx * s;
      if (qx < 0 || qx >= w) continue;
      const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
      const DnTexel cq = colour[q];
      if (cq.w == 0.0f) continue;
      const DnTexel gq = guide[q];
      const float dc = dn_dist2(cq, cp), dn = dn_dist2(gq, gp);
      const float dd = gq.w - gp.w, dz = dd * dd;
      float wt = dn_tap(dy + 2, dx + 2);
      if (kc != 0.0f) wt = wt / (1.0f + kc * dc);
      if (kn != 0.0f) wt = wt / (1.0f + kn * dn);
      if (kz != 0.0f) wt = wt / (1.0f + kz * dz);
      sr = sr + wt * cq.x;
      sg = sg + wt * cq.y;
      sb = sb + wt * cq.z;
      sumw = sumw + wt;
    }
  }
  const float r = sr / sumw, g = sg / sumw, b = sb / sumw;  // the centre tap is always taken: sumw >= 9/64
  return DnTexel{r, g, b, (dn_finite(r) && dn_finite(g) && dn_finite(b)) ? 1.0f : 0.0f};
}

// kc of level i: the colour sigma halves per level
inline float dn_level_kc(float k_color, int i) { return (float)((double)k_color * (double)(1u << (2 * i))); }

// The arguments every entry point checks the same way: NULL, or the refusal's text
inline const char* dn_check(int32_t w, int32_t h, const DrDenoiseParams* p) {
  if (!p) return "a null pointer";
  if (const char* why = img_check_dims(w, h)) return why;
  if (p->iterations < 1 || p->iterations > DR_DN_MAX_ITERATIONS) return "iterations must be in 1..8";
  const float k[3] = {p->k_color, p->k_normal, p->k_depth};
  for (int i = 0; i < 3; ++i)
    if (!dn_finite(k[i]) || k[i] < 0.0f) return "k_color, k_normal and k_depth must be finite and not negative";
  if (!dn_finite(dn_level_kc(p->k_color, p->iterations - 1))) return "k_color of the last level is not finite in f32";
  return nullptr;
}

// dn_check, the null pointers and the overlap of `out` with an input, as a refusal (`who` prefixes the message).  dr_denoise_host.cpp.
int dn_check_images(const char* who, const void* rgb, const void* normal, const void* depth, int32_t w, int32_t h,
                    const DrDenoiseParams* params, const void* out);

// What sets the a-trous filter and its pair form (dr_denoise_pair.h) apart, as the level loop of the host (dn_levels_host) and of the
// device (dr_denoise_device.hip) takes it: the images a call packs, one level's scalars, the per-pixel function, and whether the last
// level's w goes to a variance image.  Here w is the validity flag and no output.
struct DnRule {
  typedef DrDenoiseParams Params;
  typedef DnInputs Inputs;
  static constexpr bool kVariance = false;
  float kc, kn, kz;
  static DnRule level(const Params& p, int i) { return DnRule{dn_level_kc(p.k_color, i), p.k_normal, p.k_depth}; }
  DR_DN_HD DnTexel pixel(const DnTexel* colour, const DnTexel* guide, int32_t w, int32_t h, int32_t x, int32_t y, int32_t s) const {
    return dn_pixel(colour, guide, w, h, x, y, s, kc, kn, kz);
  }
};

// A call on the host is two halves, as on the device (dr_denoise_device.hip): make the two planes, run the levels.  The first half of
// the a-trous filter and of its pair form is the pack; the moments form (dr_denoise_moments.h) has a variance estimate behind it.
template <class Inputs>
void dn_pack_host(const Inputs& in, size_t n, DnTexel* colour, DnTexel* guide) {
  for (size_t p = 0; p < n; ++p) {
    colour[p] = in.colour(p);
    guide[p] = in.guide(p);
  }
}

// The levels of one call on the host: a serial loop over Rule's per-pixel function.  The levels take turns between two colour planes,
// `src` first (`dst` is not touched by a single level); the last one writes out [h][w][3] and, where the rule has one and out_var is
// set, [h][w].
template <class Rule>
void dn_run_levels_host(DnTexel* src, DnTexel* dst, const DnTexel* guide, int32_t w, int32_t h, const typename Rule::Params& prm, float* out,
                        float* out_var) {
  for (int i = 0; i < prm.iterations; ++i) {
    const bool last = i == prm.iterations - 1;
    const Rule rule = Rule::level(prm, i);
    for (int32_t y = 0; y < h; ++y)
      for (int32_t x = 0; x < w; ++x) {
        const DnTexel t = rule.pixel(src, guide, w, h, x, y, (int32_t)(1 << i));
        const size_t p = (size_t)y * (size_t)w + (size_t)x;
        if (last) {
          out[3 * p] = t.x;
          out[3 * p + 1] = t.y;
          out[3 * p + 2] = t.z;
          if (Rule::kVariance && out_var) out_var[p] = t.w;
        } else {
          dst[p] = t;
        }
      }
    std::swap(src, dst);
  }
}

// Both halves, on images that the caller has checked: the pack, then the levels
template <class Rule>
void dn_levels_host(const typename Rule::Inputs& in, int32_t w, int32_t h, const typename Rule::Params& prm, float* out, float* out_var) {
  const size_t n = (size_t)w * (size_t)h;
  std::vector<DnTexel> guide(n), a(n), b(prm.iterations > 1 ? n : 0);
  dn_pack_host(in, n, a.data(), guide.data());
  dn_run_levels_host<Rule>(a.data(), b.data(), guide.data(), w, h, prm, out, out_var);
}

#endif
