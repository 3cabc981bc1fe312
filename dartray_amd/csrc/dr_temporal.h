// dr_temporal.h -- temporal accumulation with reprojection (the temporal half of Schied et al. 2017, SVGF; the reference has no
// such stage): one pixel's rule and the parameter check, written once for the host loop (dr_temporal_host.cpp) and the device kernel
// (dr_temporal_device.hip).
//
// A call reads the current frame -- rgb, the encoded normal and the depth t along the normalised camera ray, as the feature integrator writes
// them -- and the history the previous call left: its accumulated colour, second moment of the luminance and history length, and the previous
// frame's two guides.  It rebuilds the pixel's point in the current camera's space from t, takes it to the previous camera's raster, and
// blends the current sample into the bilinear mean of the 2 x 2 previous pixels that still show that surface.
//
// Arithmetic: the geometry is f64 (+ - * /, sqrt), everything after the rounding of (u, v) to f32 is f32: + - * /, floor and comparisons, one
// operation and one rounding per operator, in the order DESIGN.md 2.23 writes them; the units that include this header are compiled with
// -ffp-contract=off and without fast-math, and `/` and sqrt are the correctly rounded ones.
#ifndef DR_TEMPORAL_H
#define DR_TEMPORAL_H

#include <math.h>

#include "dr_image.h"

#define DR_TP_MAX_HISTORY 4096

// The images of one call.  The five history pointers are all NULL on the first frame.
struct TpImages {
  const float *rgb, *normal, *depth;
  const float *h_rgb, *h_m2, *h_len, *h_normal, *h_depth;
  float *out_rgb, *out_m2, *out_len;
};

DR_DN_HD bool tp_finite(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof(u));
  return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// Row `row` of the row-major 4 x 4 matrix m times (a, b, c, 1): ((m0 * a + m1 * b) + m2 * c) + m3
DR_DN_HD double tp_row(const double* m, int row, double a, double b, double c) {
  return ((m[4 * row] * a + m[4 * row + 1] * b) + m[4 * row + 2] * c) + m[4 * row + 3];
}

// u or v: the f64 raster coordinate rounded to f32, then to the nearest 1/256 of a pixel
DR_DN_HD float tp_snap(double c) {
  const float u = (float)c;
  return __builtin_floorf(u * 256.0f + 0.5f) / 256.0f;
}

// Steps 2 and 3: where pixel (x, y)'s surface lay in the previous frame and what the previous pixels around it hold.  true: hist5 holds the
// history's r, g, b, m2 and length.  Every tap's coordinates are checked against the image before its loads.
DR_DN_HD bool tp_history(const TpImages& im, int32_t w, int32_t h, const DrTemporalParams& prm, int32_t x, int32_t y, float nx, float ny, float nz,
                         float depth, float* hist5) {
  if (!im.h_rgb) return false;
  const double rx = (double)x + 0.5, ry = (double)y + 0.5;
  const double* rc = prm.raster_to_camera;  // the raster point's z is 0: its column takes no part
  const double pw = (rc[12] * rx + rc[13] * ry) + rc[15];
  const double px = ((rc[0] * rx + rc[1] * ry) + rc[3]) / pw, py = ((rc[4] * rx + rc[5] * ry) + rc[7]) / pw,
               pz = ((rc[8] * rx + rc[9] * ry) + rc[11]) / pw;
  const double len = sqrt((px * px + py * py) + pz * pz);
  const double t = (double)depth;
  const double cx = (px / len) * t, cy = (py / len) * t, cz = (pz / len) * t;
  const double qx = tp_row(prm.cur_to_prev, 0, cx, cy, cz), qy = tp_row(prm.cur_to_prev, 1, cx, cy, cz), qz = tp_row(prm.cur_to_prev, 2, cx, cy, cz);
  const double tz = sqrt((qx * qx + qy * qy) + qz * qz);
  const double sx = tp_row(prm.prev_to_raster, 0, qx, qy, qz), sy = tp_row(prm.prev_to_raster, 1, qx, qy, qz),
               sw = tp_row(prm.prev_to_raster, 3, qx, qy, qz);
  if (!(tp_finite(qx) && tp_finite(qy) && tp_finite(qz) && tp_finite(tz) && tp_finite(sx) && tp_finite(sy) && tp_finite(sw))) return false;
  if (qz <= 0.0 || sw <= 0.0) return false;
  const double ud = sx / sw - 0.5, vd = sy / sw - 0.5;
  if (!(dn_finite((float)ud) && dn_finite((float)vd))) return false;
  const float u = tp_snap(ud), v = tp_snap(vd);
  const float lim = 16777216.0f;
  if (!(u >= -lim && u <= lim && v >= -lim && v <= lim)) return false;
  const float tzf = (float)tz, band = prm.depth_tol * tzf;
  const float fu = __builtin_floorf(u), fv = __builtin_floorf(v);
  const float tx = u - fu, ty = v - fv;
  const int64_t bx = (int64_t)fu, by = (int64_t)fv;
  const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sm = 0.0f, sl = 0.0f, sumw = 0.0f;
  for (int j = 0; j < 2; ++j) {
    const int64_t qyi = by + j;
    for (int i = 0; i < 2; ++i) {
      const int64_t qxi = bx + i;
      const float wt = wx[i] * wy[j];
      if (wt == 0.0f) continue;
      if (qxi < 0 || qxi >= w || qyi < 0 || qyi >= h) continue;
      const size_t q = (size_t)qyi * (size_t)w + (size_t)qxi;
      const float hl = im.h_len[q];
      if (!(hl > 0.0f)) continue;
      const float hz = im.h_depth[q];
      if (!dn_finite(hz)) continue;
      if (!(__builtin_fabsf(hz - tzf) <= band)) continue;
      const float hx = im.h_normal[3 * q], hy = im.h_normal[3 * q + 1], hn = im.h_normal[3 * q + 2];
      if (!(dn_finite(hx) && dn_finite(hy) && dn_finite(hn))) continue;
      const float dx = hx - nx, dy = hy - ny, dn = hn - nz;
      if (!(((dx * dx) + (dy * dy)) + (dn * dn) <= prm.normal_tol)) continue;
      const float r = im.h_rgb[3 * q], g = im.h_rgb[3 * q + 1], b = im.h_rgb[3 * q + 2], m = im.h_m2[q];
      if (!(dn_finite(r) && dn_finite(g) && dn_finite(b) && dn_finite(m))) continue;
      sr = sr + wt * r;
      sg = sg + wt * g;
      sb = sb + wt * b;
      sm = sm + wt * m;
      sl = sl + wt * hl;
      sumw = sumw + wt;
    }
  }
  if (!(sumw > 0.0f)) return false;
  hist5[0] = sr / sumw;
  hist5[1] = sg / sumw;
  hist5[2] = sb / sumw;
  hist5[3] = sm / sumw;
  hist5[4] = sl / sumw;
  return true;
}

// One pixel (x, y) of a w x h frame: its out_rgb, out_m2 and out_len.
DR_DN_HD void tp_pixel(const TpImages& im, int32_t w, int32_t h, const DrTemporalParams& prm, int32_t x, int32_t y) {
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const float r = im.rgb[3 * p], g = im.rgb[3 * p + 1], b = im.rgb[3 * p + 2];
  const float nx = im.normal[3 * p], ny = im.normal[3 * p + 1], nz = im.normal[3 * p + 2], depth = im.depth[p];
  const bool colour = dn_finite(r) && dn_finite(g) && dn_finite(b);
  const bool valid = colour && dn_finite(nx) && dn_finite(ny) && dn_finite(nz) && dn_finite(depth) && depth > 0.0f;
  const float l = img_lum(r, g, b), m2 = l * l;
  float hist[5];
  if (!valid || !tp_history(im, w, h, prm, x, y, nx, ny, nz, depth, hist)) {  // the current sample, bit for bit
    im.out_rgb[3 * p] = r;
    im.out_rgb[3 * p + 1] = g;
    im.out_rgb[3 * p + 2] = b;
    im.out_m2[p] = dn_finite(m2) ? m2 : 0.0f;
    im.out_len[p] = colour ? 1.0f : 0.0f;
    return;
  }
  const float most = (float)prm.max_history, grown = hist[4] + 1.0f;
  const float n = grown < most ? grown : most;
  const float a = 1.0f / n;
  im.out_rgb[3 * p] = hist[0] + a * (r - hist[0]);
  im.out_rgb[3 * p + 1] = hist[1] + a * (g - hist[1]);
  im.out_rgb[3 * p + 2] = hist[2] + a * (b - hist[2]);
  im.out_m2[p] = hist[3] + a * (m2 - hist[3]);
  im.out_len[p] = n;
}

// The arguments every entry point checks the same way: NULL, or the refusal's text
inline const char* tp_check(int32_t w, int32_t h, const DrTemporalParams* p) {
  if (!p) return "a null pointer";
  if (const char* why = img_check_dims(w, h)) return why;
  if (!dn_finite(p->depth_tol) || p->depth_tol < 0.0f || !dn_finite(p->normal_tol) || p->normal_tol < 0.0f)
    return "depth_tol and normal_tol must be finite and not negative";
  if (p->max_history < 1 || p->max_history > DR_TP_MAX_HISTORY) return "max_history must be in 1..4096";
  for (int i = 0; i < 16; ++i)
    if (!tp_finite(p->raster_to_camera[i]) || !tp_finite(p->cur_to_prev[i]) || !tp_finite(p->prev_to_raster[i])) return "a matrix element is not finite";
  return nullptr;
}

// tp_check, the null pointers, the partly-NULL history and the overlap of an output with an input or another output, as a refusal (`who`
// prefixes the message).  dr_temporal_host.cpp.
int tp_check_images(const char* who, const TpImages& im, int32_t w, int32_t h, const DrTemporalParams* params);

#endif
