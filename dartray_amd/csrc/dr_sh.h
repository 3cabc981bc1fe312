// dr_sh.h -- real spherical harmonics as the reference evaluates them (core/spherical_harmonics.dart: Terms, Index, Evaluate, _legendrep, _K,
// _divfact, _sinCosIndexed, ReduceRinging), shared by host and device.  Written from the reference's text, operator for operator: every
// value is an f64 and every expression keeps the reference's operand order (the units are compiled with -ffp-contract=off, so nothing fuses).
//
// lmax range: 1 <= lmax <= DR_SH_LMAX_MAX.
//   lmax < 1   is refused: _legendrep stores P(1, 0) unconditionally, so at lmax 0 the reference writes past its one-entry list.
//   lmax > 8   is refused: the diffuse PRT integrator keeps Terms(lmax) f32 transfer coefficients per camera sample in a side buffer
//               and a lane of k_shade_prt holds Terms(lmax) f64 harmonics while it folds a ray in: 81 words (324 B) per
//              slot -- twice the path state itself -- and 648 B of scratch per lane at lmax 8.  (The reference warns above 28.)
// K(l, m) depends on nothing but (l, m): sh_K_table fills Terms(lmax) doubles once with exactly what the reference's loop computes per call.
#ifndef DR_SH_H
#define DR_SH_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DR_SH_FN __host__ __device__ inline
#else
#define DR_SH_FN inline
#endif

#include <math.h>

#define DR_SH_LMAX_MAX 8
#define DR_SH_MAX_TERMS ((DR_SH_LMAX_MAX + 1) * (DR_SH_LMAX_MAX + 1))
#define DR_SH_INV_FOURPI 0.07957747154594766788  // core/common.dart:25

DR_SH_FN int sh_terms(int lmax) { return (lmax + 1) * (lmax + 1); }  // :27
DR_SH_FN int sh_index(int l, int m) { return l * l + l + m; }        // :29-30

DR_SH_FN double sh_divfact(int a, int b) {  // :738-749
  if (b == 0) return 1.0;
  const double fa = (double)a;
  const double fb = fabs((double)b);
  double v = 1.0;
  for (double x = fa - fb + 1.0; x <= fa + fb; x += 1.0) v *= x;
  return 1.0 / v;
}
DR_SH_FN double sh_K(int l, int m) { return sqrt((2.0 * l + 1.0) * DR_SH_INV_FOURPI * sh_divfact(l, m)); }  // :734-736
DR_SH_FN void sh_K_table(int lmax, double* K) {  // :46-51
  for (int l = 0; l <= lmax; ++l)
    for (int m = -l; m <= l; ++m) K[sh_index(l, m)] = sh_K(l, m);
}

// `out` is the reference's list: a List<double> (T = double) or, where the caller hands Evaluate a Float32List (Light.shProject, the lat-long
// projection), T = float -- then EVERY store rounds to f32 and the recurrences read the rounded values back, as the reference's do.
template <class T>
DR_SH_FN void sh_legendrep(double x, int lmax, T* out) {  // :685-732
  // m = 0 by recurrence
  out[sh_index(0, 0)] = (T)1.0;
  out[sh_index(1, 0)] = (T)x;
  for (int l = 2; l <= lmax; ++l) out[sh_index(l, 0)] = (T)(((2.0 * l - 1.0) * x * (double)out[sh_index(l - 1, 0)] - (l - 1) * (double)out[sh_index(l - 2, 0)]) / l);
  // the m = l edge
  double neg = -1.0;
  double dfact = 1.0;
  const double xroot = sqrt(fmax(0.0, 1.0 - x * x));
  double xpow = xroot;
  for (int l = 1; l <= lmax; ++l) {
    out[sh_index(l, l)] = (T)(neg * dfact * xpow);
    neg *= -1.0;
    dfact *= 2 * l + 1;
    xpow *= xroot;
  }
  // the m = l - 1 edge
  for (int l = 2; l <= lmax; ++l) out[sh_index(l, l - 1)] = (T)(x * (2.0 * l - 1.0) * (double)out[sh_index(l - 1, l - 1)]);
  // m = 1 .. l - 2
  for (int l = 3; l <= lmax; ++l)
    for (int m = 1; m <= l - 2; ++m)
      out[sh_index(l, m)] = (T)(((2.0 * (l - 1.0) + 1.0) * x * (double)out[sh_index(l - 1, m)] - (l - 1.0 + m) * (double)out[sh_index(l - 2, m)]) / (l - m));
}

DR_SH_FN void sh_sincos_indexed(double s, double c, int n, double* sout, double* cout) {  // :768-780
  double si = 0.0;
  double ci = 1.0;
  for (int i = 0; i < n; ++i) {
    sout[i] = si;
    cout[i] = ci;
    const double oldsi = si;
    si = si * c + ci * s;
    ci = ci * c - oldsi * s;
  }
}

// SphericalHarmonics.Evaluate(w, lmax, out) (:32-86) with K = sh_K_table(lmax).  out: Terms(lmax) doubles.  The m < 0 terms read the RAW
// Legendre value of (l, -m), which the m > 0 loop of the same band scales only afterwards, as in the reference.
template <class T>
DR_SH_FN void sh_evaluate(double wx, double wy, double wz, int lmax, const double* K, T* out) {
  sh_legendrep(wz, lmax, out);
  double sins[DR_SH_LMAX_MAX + 1], coss[DR_SH_LMAX_MAX + 1];
  const double xyLen = sqrt(fmax(0.0, 1.0 - wz * wz));
  if (xyLen == 0.0) {
    for (int i = 0; i <= lmax; ++i) sins[i] = 0.0;
    for (int i = 0; i <= lmax; ++i) coss[i] = 1.0;
  } else {
    sh_sincos_indexed(wy / xyLen, wx / xyLen, lmax + 1, sins, coss);
  }
  const double sqrt2 = sqrt(2.0);
  for (int l = 0; l <= lmax; ++l) {
    for (int m = -l; m < 0; ++m) out[sh_index(l, m)] = (T)(sqrt2 * K[sh_index(l, m)] * (double)out[sh_index(l, -m)] * sins[-m]);
    out[sh_index(l, 0)] = (T)((double)out[sh_index(l, 0)] * K[sh_index(l, 0)]);
    for (int m = 1; m <= l; ++m) out[sh_index(l, m)] = (T)((double)out[sh_index(l, m)] * (sqrt2 * K[sh_index(l, m)] * coss[m]));
  }
}

// ReduceRinging's factor of band l (:219-226; lambda = 0.005): c[Index(l, m)].scale(scale)
DR_SH_FN double sh_ringing_scale(int l, double lambda) { return 1.0 / (1.0 + lambda * l * l * (l + 1) * (l + 1)); }

#endif
