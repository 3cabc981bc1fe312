// dr_feature_value.h -- the value of a DR_FEATURE_* channel at a camera hit, written once for the two kernels that store it: k_shade_feature
// (dr_shade_feature.hip: the value is the sample's radiance) and k_guides (dr_guides.hip: the value goes to a side plane beside a beauty
// render).  What isect.dg does not carry -- (u, v) of a quadric, the default uvs of a triangle without a shading record --
// the normals' encoding and the id triple.  Both kernels run these operators in this order, so a guide plane holds the bytes the feature
// integrator's radiance would.  f64 arithmetic, one rounding to f32; the including unit is compiled with -ffp-contract=off.
// Included INSIDE the unit's layout namespace (DR_NS), behind dr_kernels.h and dr_shade_hit.h: includes nothing itself.
#ifndef DR_FEATURE_VALUE_H
#define DR_FEATURE_VALUE_H

// (u, v) of a quadric hit (sphere.dart:117-120, disk.dart:69-75) at the object-space point quadric_dg_at rebuilds (pointAt(t), the pole fix-up)
DR_DEV void feature_quadric_uv(const DQuadric& q, F3 o, F3 d, double t, double* u, double* v) {
  const F3 oo = q_point(q.w2o, o), od = q_vector(q.w2o, d);
  F3 phit = vadd(oo, vmul(od, t));
  if (q.kind == DR_QUADRIC_SPHERE && phit.x == 0.0f && phit.y == 0.0f) phit.x = (float)(1.0e-5 * q.radius);
  const double phi = q_phi(phit);
  *u = phi / q.phiMax;
  if (q.kind == DR_QUADRIC_SPHERE) {
    double r = (double)phit.z / q.radius;
    r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    const double theta = acos(r);
    *v = (theta - q.thetaMin) / (q.thetaMax - q.thetaMin);
  } else {
    const double dist2 = (double)phit.x * (double)phit.x + (double)phit.y * (double)phit.y;
    const double oneMinusV = (sqrt(dist2) - q.innerRadius) / (q.radius - q.innerRadius);
    *v = 1.0 - oneMinusV;
  }
}

// Triangle.getUVs without a uv array (triangle.dart:255-262) and the interpolation of :134-137, on the accepting test's barycentrics
DR_DEV void feature_default_uv(const Tri& tr, F3 o, F3 d, double* u, double* v) {
  double tt, b1 = 0.0, b2 = 0.0;
  (void)tri_hit(tr.p1, tr.p2, tr.p3, o, d, -DR_INF, DR_INF, &tt, &b1, &b2);
  const double b0 = 1.0 - b1 - b2;
  *u = b0 * 0.0 + b1 * 1.0 + b2 * 1.0;
  *v = b0 * 0.0 + b1 * 0.0 + b2 * 1.0;
}

// dg.u, dg.v where hit_dg does not give them: a quadric, a triangle without a shading record.  false: a triangle with one, whose hit_dg does
DR_DEV bool feature_uv_without_dg(const DScene& sc, const HitRec& h, F3 o, F3 d, double t, double* u, double* v) {
  if (h.isQuad) {
    feature_quadric_uv(sc.quads[h.tr.quad], o, d, t, u, v);
    return true;
  }
  if (!h.hasRec) {
    feature_default_uv(h.tr, o, d, u, v);
    return true;
  }
  return false;
}

DR_DEV C3 feature_normal(F3 nn) {  // 0.5 * (n + 1), per component
  return C3{(float)(0.5 * ((double)nn.x + 1.0)), (float)(0.5 * ((double)nn.y + 1.0)), (float)(0.5 * ((double)nn.z + 1.0))};
}
DR_DEV C3 feature_depth(double t) { return C3{(float)t, (float)t, (float)t}; }
DR_DEV C3 feature_uv(double u, double v) { return C3{(float)u, (float)v, 0.f}; }
// primitive + 1, material + 1, and the coverage mask
DR_DEV C3 feature_id(int prim, uint32_t mat) { return C3{(float)((double)prim + 1.0), (float)((double)mat + 1.0), 1.0f}; }

#endif
