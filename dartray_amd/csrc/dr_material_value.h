// dr_material_value.h -- the value of a DR_MATERIAL_CHANNEL_* channel for a camera ray, written once beside
// dr_feature_value.h: k_shade_material (dr_shade_material.hip) stores it as the sample's radiance, and a guide kernel that wrote material
// channels to side planes would call the same two functions and so store the same bytes.
//   material_albedo    the hit's material colour as the material's getBSDF hands it to its first lobe: Kd.evaluate(dgs).clamp() of matte
//                      (matte_material.dart:54) and plastic (plastic_material.dart:52), Kr.evaluate(dgs).clamp() of mirror
//                      (mirror_material.dart:44) and glass (glass_material.dart:52).  Constant textures: no geometry is read.
//   material_emission  what Li of the Path, DirectLighting and Whitted integrators adds for the camera ray itself
//                      (path_integrator.dart:46-48, direct_lighting_integrator.dart:40, whitted_integrator.dart:40): isect.Le(-ray.d)
//                      (intersection.dart:60-63) = DiffuseAreaLight.L(p, n, w) (diffuse_area_light.dart:44-46) with n = isect.dg.nn, the
//                      geometric normal after reverseOrientation; at a miss the sum of the lights' Le(ray) (sampler_renderer.dart:86-92):
//                      the infinite light's map (infinite_area_light.dart:84-90), every other light's 0 (light.dart:70-72).
// The colours are stored f32 values and the map lookup is env_Le's f64 with its one rounding; the including unit is compiled with
// -ffp-contract=off.  Included INSIDE the unit's layout namespace (DR_NS), behind dr_kernels.h and dr_shade_hit.h: includes nothing itself.
#ifndef DR_MATERIAL_VALUE_H
#define DR_MATERIAL_VALUE_H

// Material record (dr_device.h, make_bsdf): float4 0 = (Kd, -), float4 1 = (Kr -- plastic: Ks --, type)
DR_DEV C3 material_albedo(const DScene& sc, uint32_t mat) {
  const float4 m1 = sc.mats[4 * (size_t)mat + 1];
  const int type = (int)__float_as_uint(m1.w);
  return type == DR_MATERIAL_MIRROR || type == DR_MATERIAL_GLASS ? clamp0(m1) : clamp0(sc.mats[4 * (size_t)mat]);
}

// nn: isect.dg.nn; d: the camera ray's direction
DR_DEV C3 material_emission(const DScene& sc, const Tri& tr, F3 nn, F3 d) { return hit_Le(sc.lights, tr, nn, vneg(d)); }

#endif
