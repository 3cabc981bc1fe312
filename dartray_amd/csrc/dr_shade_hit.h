// dr_shade_hit.h -- what every shading unit outside dr_kernels.hip does with a hit, written once: the hit's geometry
// (HitRec, hit_rec, hit_dg, hit_dgs, hit_geometry), the escaped ray's Le, isect.Le, isect.rayEpsilon and Spectrum.clamp().  Outside the
// profile-pinned files (dr_kernels.hip, dr_device.h) the record-present test and the DR_SHADING_N | DR_SHADING_S test stand here only.
// Used by the dr_shade_*.hip units, inside their layout namespace (DR_NS), and by dr_probes.hip's walk at file scope.
// Behind dr_kernels.h: includes nothing itself.
#ifndef DR_SHADE_HIT_H
#define DR_SHADE_HIT_H

// ---- the hit's geometry: isect.dg and bsdf.dgShading from the ray that found the hit ----
// A primitive is a quadric, else a triangle with a shading record (its mesh has uv, N or S: word 6 of the record, its flags, is not 0),
// else a plain triangle.
struct HitRec {
  Tri tr;
  uint32_t prim;
  bool isQuad, hasRec;
};
DR_DEV HitRec hit_rec(const DScene& sc, uint32_t prim) {
  HitRec h;
  h.tr = load_tri(sc, prim);
  h.prim = prim;
  h.isQuad = h.tr.kind != 0;
  h.hasRec = !h.isQuad && sc.srec && __float_as_uint(sc.srec[7 * (size_t)prim + 6].x) != 0u;
  return h;
}
// The pieces, for a kernel that builds isect.dg and the shading geometry at different times.  It keeps the record itself
// (`const ShadeRec srec = hit_srec(sc, h);`): a HitRec that carried the record into hit_geometry cost k_shade_prt 16 bytes of scratch
// per lane and k_shade_ao seven VGPRs (MEASUREMENTS.md).
DR_DEV ShadeRec hit_srec(const DScene& sc, const HitRec& h) { return h.hasRec ? load_srec(sc, h.prim) : ShadeRec{}; }
// isect.dg of the hit at o + t d
DR_DEV void hit_dg(const DScene& sc, const HitRec& h, const ShadeRec& srec, F3 o, F3 d, double t, DGeo* dg) {
  if (h.isQuad) quadric_dg_at(sc.quads[h.tr.quad], o, d, t, dg);
  else if (h.hasRec) tri_dg_srec(h.tr, srec, o, d, t, dg);
  else tri_dg(h.tr.p1, h.tr.p2, h.tr.p3, h.tr.reverse, o, d, t, dg);
}
// shape.getShadingGeometry(dg): Triangle's for a mesh with N or S (triangle.dart:271-364), a copy elsewhere
DR_DEV void hit_dgs(const DScene& sc, const HitRec& h, const ShadeRec& srec, const DGeo& dg, DGeo* dgs) {
  if (h.hasRec && (srec.flags & (DR_SHADING_N | DR_SHADING_S))) shading_geometry(sc, srec, h.tr.reverse, dg, dgs);
  else *dgs = dg;
}
// both at once, for a kernel that needs them together: the record is loaded where it is used and lives no longer
DR_DEV void hit_geometry(const DScene& sc, const HitRec& h, F3 o, F3 d, double t, DGeo* dg, DGeo* dgs) {
  if (h.isQuad) {
    quadric_dg_at(sc.quads[h.tr.quad], o, d, t, dg);
    *dgs = *dg;
  } else if (h.hasRec) {
    const ShadeRec srec = load_srec(sc, h.prim);
    tri_dg_srec(h.tr, srec, o, d, t, dg);
    hit_dgs(sc, h, srec, *dg, dgs);
  } else {
    tri_dg(h.tr.p1, h.tr.p2, h.tr.p3, h.tr.reverse, o, d, t, dg);
    *dgs = *dg;
  }
}

// the ray left the scene: Li = sum of light.Le(ray) (sampler_renderer.dart:87-92) -- the infinite light's map, else 0
DR_DEV C3 escaped_Le(const DScene& sc, const SlotRef& sr) { return sc.hasEnv ? env_Le(sc.env, ld3f<F_RD>(sr)) : C3{0.f, 0.f, 0.f}; }
DR_DEV void store_escaped_Le(const DScene& sc, const SlotRef& sr) { stcf<F_L>(sr, escaped_Le(sc, sr)); }
// isect.Le(wo) (intersection.dart:60-63); lights: the scene's array (sc.lights) or a light view with light(i) (GlobalLights, LdsLights)
template <class L>
DR_DEV C3 hit_Le(L* lights, const Tri& tr, F3 nn, F3 wo) {
  return tr.light >= 0 ? light_L(lights[tr.light], nn, wo) : C3{0.f, 0.f, 0.f};
}
template <class LV>
DR_DEV C3 hit_Le(const LV& lv, const Tri& tr, F3 nn, F3 wo) {
  return tr.light >= 0 ? light_L(lv.light(tr.light), nn, wo) : C3{0.f, 0.f, 0.f};
}
// isect.rayEpsilon (triangle.dart:157; sphere.dart:169, disk.dart:98)
DR_DEV double ray_epsilon(bool isQuad, double t) { return (isQuad ? 5.0e-4 : 1.0e-3) * t; }
// Spectrum.clamp() with its defaults (spectrum.dart): like clamp0 (dr_device.h), but a zero of either sign becomes +0 -- clamp0 keeps -0
DR_DEV C3 clamp0_poszero(C3 c) {
  return C3{c.r < 0.f || c.r == 0.f ? 0.f : c.r, c.g < 0.f || c.g == 0.f ? 0.f : c.g, c.b < 0.f || c.b == 0.f ? 0.f : c.b};
}

#endif
