/* dartray_hip.h -- C ABI of the MI355X-native DartRay hot path.
 *
 * The reference (brendan-duncan/dartray, pure Dart) has NO native boundary; the
 * coarse Dart-level seam this library sits behind is
 *
 *     abstract class Renderer { Future<OutputImage> render(Scene scene); ... }
 *                                              (lib/core/renderer.dart:27-35)
 *
 * called once per task from DartRay.worldEnd (lib/dartray/dartray.dart:574).
 * A Dart `HipSamplerRenderer extends Renderer` flattens the
 * Scene (BVHAccel.nodes/primitives are public fields, bvh_accel.dart:486-487,
 * :533-538) into the POD structs below and calls these entry points through
 * dart:ffi.  Every entry point cites the reference interface it replaces.
 *
 * Conventions: plain C, POD structs, little endian.  The caller owns every
 * host buffer for the duration of the call; the library owns device memory.
 * All functions return DR_OK (0) or a negative error code; dr_last_error()
 * gives the message (the Dart shim turns it into LogSevere -> Exception ->
 * completeError, log.dart:42-47, dartray.dart:573-583).  Calls are blocking
 * unless they take a stream.  One DrScene per GPU / rank, one calling thread
 * per DrScene.
 */
#ifndef DARTRAY_HIP_H
#define DARTRAY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_OK 0
#define DR_ERR_INVALID (-1)
#define DR_ERR_HIP (-2)
#define DR_ERR_NO_DEVICE (-3)
#define DR_ERR_UNSUPPORTED (-4)

/* _LinearBVHNode (lib/accelerators/bvh_accel.dart:533-538): bounds, offset
 * (first primitive for a leaf, second-child index for an interior node; the
 * first child is index+1, :432), nPrimitives (0 => interior), split axis. */
typedef struct DrBvhNode {
  float bmin[3];
  float bmax[3];
  uint32_t offset;
  uint16_t nprims;
  uint8_t axis;
  uint8_t pad;
} DrBvhNode; /* 32 bytes */

/* MatteMaterial with constant textures (lib/materials/matte_material.dart:41-65). */
#define DR_MATERIAL_MATTE 0  /* MatteMaterial (lib/materials/matte_material.dart): kd, sigma */
#define DR_MATERIAL_MIRROR 1 /* MirrorMaterial (mirror_material.dart:38-55): kr */
#define DR_MATERIAL_GLASS 2  /* GlassMaterial (glass_material.dart:44-69): kr, kt, index */
#define DR_MATERIAL_PLASTIC 3 /* PlasticMaterial (plastic_material.dart:43-70): kd, ks in kr, roughness in index */
typedef struct DrMaterial {
  int32_t type; /* DR_MATERIAL_*; specular materials are traced by the PathIntegrator only */
  float kd[3];
  float kr[3];
  float kt[3];
  double sigma; /* matte: 0 => Lambertian, else OrenNayar(Kd, sigma) (matte_material.dart:54-61); a Dart double */
  double index; /* glass: the constant 'index' texture's value (a Dart double) */
} DrMaterial;

#define DR_LIGHT_DIFFUSE_AREA 0 /* DiffuseAreaLight (lib/lights/diffuse_area_light.dart) */
#define DR_LIGHT_INFINITE 1     /* InfiniteAreaLight (lib/lights/infinite_area_light.dart) */
#define DR_LIGHT_POINT 2        /* PointLight (lib/lights/point_light.dart): a delta light */
#define DR_LIGHT_SPOT 3         /* SpotLight (lib/lights/spot_light.dart): a delta light */
#define DR_LIGHT_DISTANT 4      /* DistantLight (lib/lights/distant_light.dart): a delta light */
#define DR_LIGHT_SPOT_COS 5     /* DR_LIGHT_SPOT whose cone_width / cone_falloff_start hold the two COSINES a constructed SpotLight
                                 * keeps (cosTotalWidth, cosFalloffStart: spot_light.dart:46-47) instead of the constructor's
                                 * degrees -- what a host that only sees the Light object can marshal bit for bit */

/* One entry of Scene.lights.  kind DR_LIGHT_DIFFUSE_AREA: DiffuseAreaLight + its
 * ShapeSet (diffuse_area_light.dart:36-43, lib/core/light/shape_set.dart:24-51);
 * the triangle list is in ShapeSet order (i.e. after the LIFO refine
 * reversal).  kind DR_LIGHT_INFINITE: InfiniteAreaLight; L is the factor
 * _radiance() applies (infinite_area_light.dart:180-182), env_index selects the
 * radiance map. */
typedef struct DrAreaLight {
  float L[3];
  int32_t nsamples;
  uint32_t first_tri; /* into light_tris */
  uint32_t ntris;
  uint32_t kind;
  uint32_t env_index; /* into env_maps */
  float position[3];  /* DR_LIGHT_POINT / _SPOT: lightPos = lightToWorld(0,0,0) (point_light.dart:36-39); L = intensity.
                       * DR_LIGHT_DISTANT: lightDir = normalize(lightToWorld(dir)) (distant_light.dart:38-42); L = radiance */
  float pad;
  float world_to_light[16];  /* DR_LIGHT_SPOT: Light.worldToLight (falloff is evaluated in light space, spot_light.dart:54-70) */
  double cone_width, cone_falloff_start;  /* DR_LIGHT_SPOT: total width and falloff start, degrees (spot_light.dart:42-48) */
} DrAreaLight;

/* InfiniteAreaLight's radiance map (f32 RGB texels, TEXTURE_REPEAT) and Light.lightToWorld / worldToLight
 * (lib/core/light.dart:28-34).  texels: either level 0 of the light's MIPMap (MIPMap.pyramid[0], lib/core/mipmap.dart:139 -- always
 * a power-of-two size) or the image as MIPMap.texture receives it (already multiplied by L, infinite_area_light.dart:44-49): a width
 * or height that is no power of two is resampled up to the next one exactly as that constructor does (mipmap.dart:71-138: four-tap
 * Lanczos, s then t, clamped at 0).  The Distribution2D over luminance x sin(theta) (infinite_area_light.dart:283-307) is rebuilt by
 * the library.  At most 16384 texels a side. */
typedef struct DrEnvMap {
  const float* texels; /* [height][width][3] */
  int32_t width, height;
  float light_to_world[16];
  float world_to_light[16];
} DrEnvMap;

typedef struct DrLightTri {
  uint32_t v[3]; /* vertex indices; v[0] == DR_PRIM_QUADRIC: v[1] indexes DrSceneDesc.quadrics */
  uint32_t reverse_orientation; /* bit 0: Shape.reverseOrientation; bit 1: the mesh has uvs (vert_uvs) */
} DrLightTri;

/* objectToWorld of a TriangleMesh that carries per-vertex normals / tangents: they stay in object space and are
 * transformed at shading time (lib/shapes/triangle.dart:303-317). */
typedef struct DrMeshXform {
  float object_to_world[16];
  float world_to_object[16];
} DrMeshXform;
#define DR_SHADING_N 1u  /* tri_shading bits: the primitive's mesh has 'N' */
#define DR_SHADING_S 2u  /* ... 'S' */
#define DR_SHADING_UV 4u /* ... 'uv' / 'st' */

/* Quadric shapes (lib/shapes/sphere.dart:23-38, lib/shapes/disk.dart:23-29).  Unlike triangle meshes they keep
 * their objectToWorld Transform and transform the RAY per test (transform.dart:180-196).  A primitive whose
 * tri_idx[3*i] is DR_PRIM_QUADRIC is the quadric tri_idx[3*i+1]; its material / light / orientation come from
 * the same per-primitive tables as a triangle's. */
#define DR_PRIM_QUADRIC 0xFFFFFFFFu
#define DR_QUADRIC_SPHERE 1
#define DR_QUADRIC_DISK 2
typedef struct DrQuadric {
  int32_t kind; /* DR_QUADRIC_* */
  int32_t pad;
  float object_to_world[16]; /* Shape.objectToWorld.m, row-major */
  float world_to_object[16]; /* Shape.objectToWorld.mInv == worldToObject.m (dartray.dart:383-384) */
  /* constructor arguments as Dart doubles -- sphere: radius, z0, z1, phimax [deg] (sphere.dart:313-321);
   * disk: height, radius, innerradius, phimax [deg] (disk.dart:157-165) */
  double params[4];
} DrQuadric;

/* Flattened Scene (lib/core/scene.dart:26-45): aggregate + lights. */
typedef struct DrSceneDesc {
  const DrBvhNode* nodes; /* BVHAccel.nodes, depth-first (bvh_accel.dart:419-437) */
  uint64_t nnodes;
  const float* verts; /* world-space f32 xyz (lib/shapes/triangle_mesh.dart:29-36) */
  uint64_t nverts;
  const uint32_t* tri_idx; /* ntris*3, BVHAccel.primitives order */
  uint64_t ntris;
  const uint32_t* tri_material; /* per primitive: index into materials */
  const int32_t* tri_light;     /* per primitive: area-light index or -1 (geometric_primitive.dart:63-65) */
  const uint8_t* tri_reverse;   /* per primitive: Shape.reverseOrientation (shape.dart:29) */
  const DrMaterial* materials;
  uint32_t nmaterials;
  const DrAreaLight* lights; /* Scene.lights order */
  uint32_t nlights;
  const DrLightTri* light_tris;
  uint32_t nlight_tris;
  uint32_t bvh_depth; /* max depth of the tree; 0 = unknown: dr_scene_create measures it */
  const DrEnvMap* env_maps; /* at most one infinite light is supported */
  uint32_t nenv_maps;
  const DrQuadric* quadrics; /* spheres / disks referenced from tri_idx and light_tris */
  uint32_t nquadrics;
  /* optional per-vertex shading data (triangle_mesh.dart:195-203; Triangle.getShadingGeometry triangle.dart:271-364,
   * Triangle.getUVs :247-263): arrays indexed like verts (entries of meshes without the attribute are ignored),
   * and per primitive which attributes its mesh has / which transform it uses.  All NULL: no mesh has any. */
  const float* vert_normals;   /* nverts*3, OBJECT space */
  const float* vert_tangents;  /* nverts*3, OBJECT space */
  const float* vert_uvs;       /* nverts*2 */
  const uint8_t* tri_shading;  /* ntris: DR_SHADING_* bits */
  const uint32_t* tri_xform;   /* ntris: index into mesh_xforms (read when DR_SHADING_N or _S is set) */
  const DrMeshXform* mesh_xforms;
  uint32_t nmesh_xforms;
} DrSceneDesc;

typedef struct DrScene DrScene;

/* Ray (lib/core/ray.dart:27-47) and the hit record of
 * GeometricPrimitive.intersect (geometric_primitive.dart:47-61). */
typedef struct DrRay {
  float o[3];
  float d[3];
  double tmin;
  double tmax;
} DrRay;

typedef struct DrHit {
  int32_t prim; /* index in BVH primitive order; -1 = miss.  any-hit: 0 = occluded, -1 = free */
  int32_t pad;
  double t;
  double b1;
  double b2;
} DrHit;

/* Camera state (lib/core/projective_camera.dart:27-32): PerspectiveCamera (cameras/perspective_camera.dart:93-132),
 * OrthographicCamera (cameras/orthographic_camera.dart:52-80) -- both ProjectiveCameras with their own
 * raster_to_camera -- and EnvironmentCamera (cameras/environment_camera.dart:42-52), which only uses camera_to_world
 * and the film resolution. */
#define DR_CAMERA_PERSPECTIVE 0
#define DR_CAMERA_ORTHOGRAPHIC 1
#define DR_CAMERA_ENVIRONMENT 2
typedef struct DrCamera {
  float raster_to_camera[16]; /* row-major, Matrix4x4.data order (matrix4x4.dart:170-176) */
  float camera_to_world[16];
  double lens_radius;    /* ProjectiveCamera.lensRadius / focalDistance and Camera.shutterOpen / shutterClose are Dart */
  double focal_distance; /* doubles (projective_camera.dart:31-32, camera.dart): a lens radius of 0.8 is 0.8, not its */
  double shutter_open;   /* f32 neighbour                                                                          */
  double shutter_close;
  int32_t type; /* DR_CAMERA_* */
  int32_t pad;
} DrCamera;

/* ImageFilm + Filter (lib/film/image_film.dart:51-97). */
typedef struct DrFilm {
  int32_t xres, yres;
  double crop[4];              /* cropWindow: Dart doubles (image_film.dart:61-65 rounds xres * crop up) */
  double filter_xw, filter_yw; /* Filter.xWidth / yWidth (filter.dart:33-37), Dart doubles */
  float filter_table[256];     /* 16x16, image_film.dart:74-82 */
} DrFilm;

#define DR_INTEGRATOR_DIRECT_ALL 0 /* DirectLightingIntegrator, strategy "all" (direct_lighting_integrator.dart) */
#define DR_INTEGRATOR_PATH 1       /* PathIntegrator (path_integrator.dart) */
#define DR_INTEGRATOR_DIRECT_ONE 2 /* DirectLightingIntegrator, strategy "one" (direct_lighting_integrator.dart:51-55,82-87): ONE light per
                                    * vertex, picked by its own 1-D sample slot (lightNumOffset), the estimate scaled by the light count */
/* WhittedIntegrator (whitted_integrator.dart:26-72): at every hit Le, ONE light sample per light -- the light half only, no
 * BSDF-sampling half, no MIS weight, no nsamples -- and SpecularReflect / SpecularTransmit while ray.depth + 1 < max_depth.  It requests no sample
 * slots: the vector is image, lens, time and the volume integrator's two 1-D slots (dr_sample_floats: 7), and every LightSample.random(rng) is
 * three draws of the sample's keyed in-Li stream (kind 2) in EVERY sampler mode, DR_SAMPLER_HOST_BUFFER included (tail / max_tail are not read:
 * a ray tree's draws have no useful bound).  max_depth < 1 is DR_ERR_INVALID, DR_SAMPLER_ADAPTIVE with it DR_ERR_UNSUPPORTED; every other sampler
 * mode is served.  One count is read back per round of the specular recursion, as for DirectLighting over mirror / glass. */
#define DR_INTEGRATOR_WHITTED 3
/* AmbientOcclusionIntegrator (ambient_occlusion_integrator.dart:28-53): at the camera hit nsamples occlusion rays
 * Ray(p, w, mindist, maxdist) over the hemisphere of the geometric normal facing the camera ray -- w = UniformSampleSphere(Sample02(i, scramble)),
 * negated where Dot(w, n) < 0 -- and the radiance Spectrum(nClear / nsamples), nClear the rays scene.intersectP does not stop.  Its three
 * parameters travel in DrRenderDesc.ao_nsamples / ao_mindist / ao_maxdist; max_depth is not read.  It requests no sample slots
 * (dr_sample_floats: 7) and the two rng.randomUint() of the scramble are draws 0 and 1 of the sample's keyed in-Li stream (kind 2) in EVERY
 * sampler mode, DR_SAMPLER_HOST_BUFFER included (seed keys them; there is no recorded tail).  ao_nsamples is rounded up to a power of two as the
 * constructor does; below 1 or above 4096 after rounding, ao_mindist < 0 (or NaN) and ao_maxdist <= ao_mindist (or NaN) are DR_ERR_INVALID,
 * DR_SAMPLER_ADAPTIVE with it DR_ERR_UNSUPPORTED; every other sampler mode is served.  The scene needs no light.  No host wait: the number of rounds
 * of the stage loop (128 rays each) is known up front. */
#define DR_INTEGRATOR_AO 4
/* The first-hit feature integrator (the reference has none): the radiance of a sample is one quantity of the camera
 * ray's Intersection, chosen by DrRenderDesc.feature_channel -- a guide image (normal, depth, uv, ids) that goes through the same sampler,
 * filter, tiles and shards as the beauty image and is aligned with it sample for sample.  A camera ray that hits nothing gives 0, 0, 0; no
 * light is read (a scene without lights renders), max_depth is not read, no sample slots are requested (dr_sample_floats: 7) and nothing is
 * drawn inside Li (a host-buffer replay needs neither tail nor seed).  One stage, no ray beyond the camera's.  An unknown channel is
 * DR_ERR_INVALID, DR_SAMPLER_ADAPTIVE with it DR_ERR_UNSUPPORTED, DR_FEATURE_ID over a scene of 2^24 primitives or more DR_ERR_UNSUPPORTED
 * (dr_feature_check says so without a scene); every other sampler mode is served. */
#define DR_INTEGRATOR_FEATURE 5
/* DiffusePRTIntegrator (diffuse_prt_integrator.dart:23-92 with core/spherical_harmonics.dart): soft environment and area
 * lighting with self-shadowing from occlusion rays only.  Once per scene and lmax the lights' direct radiance at the centre of the world bound
 * is projected onto (lmax + 1)^2 spherical harmonics (dr_prt_incident returns these coefficients); at every camera hit prt_nsamples rays
 * Ray(p, w, rayEpsilon), w = UniformSampleSphere(Sample02(i, scramble)) with Dot(w, n) > 0 for the SHADING normal n facing the camera ray, project
 * the cosine-weighted visibility onto the same basis, and Li = Le + Kd * clamp(dot of the two).  Its parameters travel in
 * DrRenderDesc.prt_nsamples / prt_lmax; max_depth is not read.  It requests no sample slots (dr_sample_floats: 7) and the two randomUint() of the
 * scramble are draws 0 and 1 of the sample's keyed in-Li stream (kind 2) in EVERY sampler mode, DR_SAMPLER_HOST_BUFFER included.  prt_nsamples is
 * rounded up to a power of two as the constructor does; below 1 or above 4096, prt_lmax below 1 or above 8 are DR_ERR_INVALID; a scene with a
 * material other than matte with sigma 0 and DR_SAMPLER_ADAPTIVE are DR_ERR_UNSUPPORTED, by name.  No host wait between the rounds of 128 rays. */
#define DR_INTEGRATOR_DIFFUSE_PRT 7 /* (6 stays unassigned: dr_sample_floats and dr_render* keep answering it as they answer every unknown value) */
/* GlossyPRTIntegrator (glossy_prt_integrator.dart:23-134 with core/spherical_harmonics.dart): view-dependent highlights
 * under soft environment and area light, from occlusion rays only.  Once per scene the incident light c_in (as for DR_INTEGRATOR_DIFFUSE_PRT)
 * and the BSDF matrix B of Lambertian(Kd) + Microfacet(Ks, FresnelDielectric(1.5, 1), Blinn(1 / roughness)) over 1024 x 1024 direction pairs
 * (dr_scene_set_glossy_prt sets Kd, Ks, roughness; dr_prt_bsdf_matrix returns B); at every camera hit prt_nsamples rays Ray(p, w, rayEpsilon),
 * w = UniformSampleSphere(Sample02(i, scramble)) -- every one traced -- give the transfer matrix T, and
 * Li = Le + clamp(sum_i (B . Rotate(T . c_in))[i] * Ylm_i(woLocal)), Rotate being the reference's (its lists share objects: DESIGN.md,
 * "Reference quirks that are reproduced").  Parameters in DrRenderDesc.prt_nsamples / prt_lmax; max_depth is not read; no sample slots
 * (dr_sample_floats: 7); the scramble's two randomUint() are draws 0 and 1 of the sample's keyed in-Li stream (kind 2) in every sampler mode.
 * prt_nsamples is rounded up to a power of two; below 1 or above 4096, prt_lmax below 1 or above 4 are DR_ERR_INVALID; DR_SAMPLER_ADAPTIVE is
 * DR_ERR_UNSUPPORTED, by name.  It reads no material function, so no material is refused. */
#define DR_INTEGRATOR_GLOSSY_PRT 9 /* (8, like 6, stays unassigned and is answered as every unknown value is) */
/* UseProbesIntegrator (use_probes_integrator.dart:23-185): Li = Le + rho * INV_PI * clamp(E(n)), E the irradiance
 * function of the scene's radiance-probe grid (dr_scene_set_probes) interpolated trilinearly at the hit and convolved with the clamped cosine.
 * One shading launch (k_shade_probes) behind the camera rays, no further ray.  Its sample slots are the scene's DirectLighting "all" slots
 * (requestSamples asks for them; Li does not read them).  No grid on the scene: DR_ERR_INVALID; a grid with includeDirect 0, a material other
 * than matte with sigma 0, DR_SAMPLER_ADAPTIVE: DR_ERR_UNSUPPORTED, by name.  max_depth is not read. */
#define DR_INTEGRATOR_USE_PROBES 11 /* (10, like 6 and 8, stays unassigned) */
/* The first-hit material integrator (the reference has none): the feature integrator's sibling for the two quantities
 * that integrator does not have because it reads no material and no light by contract.  The radiance of a sample is, by
 * DrRenderDesc.material_channel, the camera hit's material colour (albedo) or what Li of the Path, DirectLighting and Whitted integrators adds
 * for the camera ray itself (emission: isect.Le(-ray.d) at a hit, the sum of the lights' Le(ray) at a miss) -- noise-free images aligned with
 * the beauty image sample for sample, which dr_demodulate* takes out of it ahead of the filters.  max_depth is not read, no sample slots are
 * requested (dr_sample_floats: 7), nothing is drawn inside Li.  One stage, no ray beyond the camera's.  An unknown channel is DR_ERR_INVALID
 * (dr_material_check says so without a scene), DR_SAMPLER_ADAPTIVE with it DR_ERR_UNSUPPORTED; every other sampler mode is served. */
#define DR_INTEGRATOR_MATERIAL 13 /* (12, like 6, 8 and 10, stays unassigned) */
/* DrRenderDesc.feature_channel: R, G, B at a hit.  Every value is >= 0 (the renderer blacks out a sample of negative luminance). */
#define DR_FEATURE_NG 0    /* 0.5 * (isect.dg.nn + 1): the geometric normal, world space, reverseOrientation applied */
#define DR_FEATURE_NS 1    /* 0.5 * (bsdf.dgShading.nn + 1): Triangle.getShadingGeometry (per-vertex N / S); else the geometric one */
#define DR_FEATURE_DEPTH 2 /* t, t, t: the camera ray's parameter at the hit (ray.maxDistance after scene.intersect) */
#define DR_FEATURE_UV 3    /* dg.u, dg.v, 0 */
#define DR_FEATURE_ID 4    /* primitive index + 1, material index + 1, 1 (indices of dr_scene_create's arrays); B is the coverage mask.
                            * Meaningful per sample, or with a box filter of width 0.5 at 1 spp: any other film averages ids */
/* DrRenderDesc.material_channel: R, G, B of a camera sample.  Every value is >= 0 for colours and radiances that are. */
#define DR_MATERIAL_CHANNEL_ALBEDO 0   /* the hit's material colour after Spectrum.clamp(): Kd of matte and plastic, Kr of mirror and glass; a miss: 0 */
#define DR_MATERIAL_CHANNEL_EMISSION 1 /* isect.Le(-ray.d): Lemit of the hit's area light where Dot(dg.nn, -ray.d) > 0, else 0; a miss: the lights' Le(ray) */

#define DR_SAMPLER_HOST_BUFFER 0 /* caller supplies sample vectors (+ the in-Li RNG draws) */
#define DR_SAMPLER_COUNTER 1     /* on-device LD sampler, keyed per (pixel, block) / (pixel, sample) */
/* On-device StratifiedSampler (stratified_sampler.dart:67-124) on keyed streams: one per pixel (the jittered image / lens / time strata
 * and the two shuffles) and one per (pixel, sample) (the LatinHypercube draws of the integrator's slots); DESIGN.md section 2.7.
 * spp = xsamples * ysamples with xsamples = DrRenderDesc.strat_xsamples; spp must be a power of two (<= 4096), and under
 * DR_INTEGRATOR_DIRECT_ALL every light's nsamples must be a power of two as well (StratifiedSampler.roundSize is the identity, the scene's slot layout
 * is the rounded one): DR_ERR_UNSUPPORTED otherwise.  _NOJITTER: `jitter false` -- every stratum's centre; the shuffles and the
 * LatinHypercube draws stay random. */
#define DR_SAMPLER_STRATIFIED 2
#define DR_SAMPLER_STRATIFIED_NOJITTER 3
/* On-device AdaptiveSampler (adaptive_sampler.dart:101-187, method "contrast", FULL_SAMPLING) on the keyed streams of DR_SAMPLER_COUNTER;
 * DESIGN.md section 2.8.  Pass 1 traces every pixel of the call's window exactly as DR_SAMPLER_COUNTER does at minSamples.  A pixel whose
 * samples' luminances (after the renderer's NaN / negative / infinite guards) satisfy |lum_i - Lavg| / Lavg > 0.5 for some i (f64, Lavg summed
 * in sample order; a black pixel never does) is traced again exactly as DR_SAMPLER_COUNTER does at maxSamples, and ONLY that second set reaches
 * the film: film == counter render of the other pixels at minSamples + counter render of these at maxSamples.  maxSamples = DrRenderDesc.spp,
 * minSamples = DrRenderDesc.strat_xsamples; both powers of two, 2 <= minSamples < maxSamples <= 4096 (the host applies the constructor's
 * swapping / rounding / doubling, adaptive_sampler.dart:53-83): DR_ERR_INVALID otherwise.  Method "shapeid" does not exist here (the camera
 * hit's ids are not kept per sample).  One host round trip per call (the number of flagged pixels); dr_scene_get_adaptive_pixels lists them. */
#define DR_SAMPLER_ADAPTIVE 4
/* On-device HaltonSampler (halton_sampler.dart:31-104); DESIGN.md section 2.9.  The samples belong to the IMAGE, not to a pixel: with
 * (left, top, width, height) the call's task window of the sampler extent and delta = max(width, height), index k of the task's own sequence,
 * k in [0, spp * delta * delta), lands at imageX = Lerp(RadicalInverse(k, 3), left, left + delta), imageY = Lerp(RadicalInverse(k, 2), top,
 * top + delta) (f64) and is REJECTED iff imageX > left + width - 1 || imageY > top + height - 1; lens and time are the radical inverses of
 * k + 1 in bases 5, 7, 11 (the reference's increment comes first), the integrator's slots LatinHypercube draws on the keyed stream
 * (seed, k, 0, kind 5), the draws inside Li the stream (seed, k, 0, kind 2).  Pixels receive different numbers of samples.
 * DrRenderDesc.spp = pixelsamples: ANY integer >= 1 (DR_ERR_INVALID otherwise); strat_xsamples is ignored.  A task owns its own sequence over
 * its own sub-window (task_num / task_count), as the reference builds one sampler per task; tile_count > 1 is DR_ERR_UNSUPPORTED (tiles deal out
 * pixels), and so are spp * delta^2 >= 2^53 (or 2^31 rows of the sampler extent: the in-Li streams are keyed by the index as a pixel of the
 * extent) and, under DR_INTEGRATOR_DIRECT_ALL, a light whose nsamples is no power of two (roundSize is the
 * identity).  Departure from the reference, as for every sample vector here: image fraction, lens and time are rounded to f32 once (the image
 * sample by at most 2^-25 pixel).  One host wait per batch of the call (the number of accepted samples of the batch's index range).
 * DrRenderStats.camera_samples counts the accepted samples, film_samples the window's film pixels x spp. */
#define DR_SAMPLER_HALTON 5
/* On-device RandomSampler (random_sampler.dart:47-88, FULL_SAMPLING); DESIGN.md section 2.11.  One keyed stream per (pixel, sample),
 * (seed, pixelIndex, sample, kind 6) with pixelIndex the pixel's position in the full sampler extent; every value of the sample vector is one
 * Random.nextDouble() of it, in the reference's order: image x, image y, lens u, lens v, time, then the entries of every 1-D slot and of every
 * 2-D slot in request order.  Nothing is stratified, shuffled or permuted; the draws inside Li stay on kind 2 as in every mode.
 * DrRenderDesc.spp = pixelsamples, a power of two <= 4096 (the reference's default of 10 has to be given as a power of two), and under
 * DR_INTEGRATOR_DIRECT_ALL every light's nsamples must be a power of two (RandomSampler.roundSize is the identity, the scene's slot layout is
 * the rounded one): DR_ERR_UNSUPPORTED otherwise.  strat_xsamples is ignored.  Departure from the reference, as for DR_SAMPLER_HALTON: image
 * fraction, lens and time are rounded to f32 once (the image sample by at most 2^-25 pixel); the slots' values are exact. */
#define DR_SAMPLER_RANDOM 6

/* Everything SamplerRenderer.render needs besides the Scene
 * (lib/renderers/sampler_renderer.dart:29-31,36-65). */
typedef struct DrRenderDesc {
  DrCamera camera;
  DrFilm film;
  int32_t integrator;
  int32_t max_depth; /* PathIntegrator.maxDepth / DirectLightingIntegrator.maxDepth / WhittedIntegrator.maxDepth (default 5) */
  int32_t spp;       /* LowDiscrepancySampler.nPixelSamples, StratifiedSampler's xPixelSamples * yPixelSamples or AdaptiveSampler.maxSamples, power of two;
                      * DR_SAMPLER_HALTON: pixelsamples, any integer >= 1; DR_SAMPLER_RANDOM: pixelsamples, a power of two */
  int32_t sampler_mode;
  int64_t seed; /* the device samplers' keyed streams; DR_INTEGRATOR_WHITTED: its in-Li streams in every sampler mode, DR_SAMPLER_HOST_BUFFER too */
  /* Work split.  task_*: the reference's GetSubWindow rectangle of the sampler
   * window (lib/core/common.dart:52-73, dartray.dart:1009-1023).  tile_*: 32x32
   * tiles (TilePixelSampler.tileSize, tile_pixel_sampler.dart:37) dealt
   * round-robin over ranks; tile_count <= 1 disables it. */
  int32_t task_num, task_count;
  int32_t tile_rank, tile_count, tile_size;
  int32_t strat_xsamples; /* DR_SAMPLER_STRATIFIED(_NOJITTER): xPixelSamples; yPixelSamples = spp / strat_xsamples, exactly.
                           * DR_SAMPLER_ADAPTIVE: the field doubles as AdaptiveSampler.minSamples.  Else ignored */
  /* DR_SAMPLER_HOST_BUFFER: nsamples camera samples, in reference order
   * (pixel-major, all spp of a pixel adjacent). */
  int64_t nsamples;
  const int32_t* pixel_xy;  /* [nsamples/spp][2] raster pixel of each group of spp samples */
  const float* sample_vec;  /* [nsamples][sample_stride]: imageU, imageV, lensU, lensV, time, oneD..., twoD... */
  int32_t sample_stride;
  union {
    int32_t ao_nsamples;    /* DR_INTEGRATOR_AO: AmbientOcclusionIntegrator's ns (the former padding at offset 1324: read under that integrator only) */
    int32_t prt_nsamples;   /* DR_INTEGRATOR_DIFFUSE_PRT / DR_INTEGRATOR_GLOSSY_PRT: the integrator's ns (reference default 4096), read under those two only */
  };
  /* DR_INTEGRATOR_AO draws from keyed streams in every sampler mode and reads no tail: under it, and only under it, the storage of the two tail
   * pointers carries AmbientOcclusionIntegrator.minDist / maxDist (Dart doubles).  Under every other integrator the unions are `tail` and
   * `tail_offsets` as they always were: same names, same offsets, same meaning. */
  union {
    const double* tail;     /* [nsamples][max_tail] RNG.randomFloat() values drawn inside Li, or NULL */
    double ao_mindist;      /* DR_INTEGRATOR_AO: minDist (reference default 1e-4) */
  };
  int32_t max_tail;
  union {
    int32_t feature_channel; /* DR_INTEGRATOR_FEATURE: DR_FEATURE_* (the former padding at offset 1340: read under that integrator only) */
    int32_t prt_lmax;        /* DR_INTEGRATOR_DIFFUSE_PRT: lmax, 1 .. 8; DR_INTEGRATOR_GLOSSY_PRT: 1 .. 4 (reference default 4), read under those two only */
    int32_t material_channel; /* DR_INTEGRATOR_MATERIAL: DR_MATERIAL_CHANNEL_*, read under that integrator only */
  };
  /* Optional packed form of `tail` (round 5): tail_offsets[nsamples + 1], non-decreasing; sample s owns
   * tail[tail_offsets[s] .. tail_offsets[s + 1]) -- the values it actually drew, in draw order (position p of the fixed
   * form = element p of the run; a read past the run yields 0.0 like the zero fill of the fixed form); max_tail stays the
   * bound on a run's length.  NULL: the fixed [nsamples][max_tail] form.  A path draws nothing before its fourth vertex
   * and most paths end early, so a recorded C2 stream holds ~5 of its 40 slots per sample: the replay moves 0.4 x the
   * bytes over PCIe. */
  union {
    const uint64_t* tail_offsets;
    double ao_maxdist;      /* DR_INTEGRATOR_AO: maxDist (reference default: infinity) */
  };
} DrRenderDesc;

/* Counters and timings accumulated over the dr_render* calls on a scene since
 * the last dr_reset_stats (the "Stats" probes of lib/core/stats.dart that the
 * hot loops call, e.g. bvh_accel.dart:106-163). */
typedef struct DrRenderStats {
  uint64_t camera_samples; /* samples traced (incl. the sampler's dead border, image_film.dart:247-252) */
  uint64_t film_samples;   /* film pixels in this rank's window x spp: the throughput numerator */
  uint64_t closest_rays, any_rays;
  uint64_t closest_nodes, any_nodes; /* iterations of the loops at bvh_accel.dart:122 / :185 */
  uint64_t closest_tris, any_tris;   /* primitive tests at bvh_accel.dart:131 / :193 */
  uint64_t trace_launches;           /* number of traversal-kernel launches (closest + any) */
  double trace_ms;                   /* summed device time of the traversal launches (HIP events) */
  double total_ms;                   /* device time of the render calls (HIP events) */
  uint64_t batches;
  uint64_t closest_launches, any_launches; /* per kernel: k_trace<0> (closest hit), k_trace<1> (any hit) */
  double closest_ms, any_ms; /* a stage's any-hit launch runs beside its closest-hit launch (second stream; DARTRAY_OVERLAP_ANY=0
                              * serialises them): any_ms counts its time AFTER the closest-hit launch ended */
  double shade_ms;  /* k_shade_path / k_shade_direct */
  double gen_ms;    /* k_gen_samples (+ host-buffer transpose) and k_raygen */
  double film_ms;   /* k_film */
  /* shading-stage work items, summed over the stages of every batch: entries of the stage's active list
   * (shade_items), of which path vertices that were set up (a surface hit within maxDepth: shade_vertices), and
   * the rays they queued (continuation, MIS and shadow rays) */
  uint64_t shade_items, shade_vertices, shade_cont, shade_mis, shade_shadow;
  /* device time of the traversal-kernel pilot the FIRST big render of a big scene runs (dr_render_device); it is
   * part of that call's total_ms */
  double pilot_ms;
} DrRenderStats;

/* Select the GPU.  Must precede everything else. */
int dr_init(int device);

/* Host-side BVHAccel constructor (bvh_accel.dart:41-91,228-437; SAH, 12
 * buckets): used by the standalone host; a Dart caller marshals its own
 * BVHAccel.nodes instead.  tri_idx is in *refined* primitive order.
 * nodes_out holds 2*ntris-1 nodes; order_out[i] = input triangle placed at
 * BVH primitive slot i. */
int dr_bvh_build(const float* verts, uint64_t nverts, const uint32_t* tri_idx, uint64_t ntris, int32_t max_prims_in_node,
                 DrBvhNode* nodes_out, uint64_t* nnodes_out, uint32_t* order_out, uint32_t* depth_out);

/* Same with quadric primitives in the list: a row tri_idx[3*i] == DR_PRIM_QUADRIC takes its world bound
 * (Shape.worldBound, shape.dart:37-39) from quadric_bounds[6 * tri_idx[3*i+1]] = (pMin xyz, pMax xyz). */
int dr_bvh_build_mixed(const float* verts, uint64_t nverts, const uint32_t* tri_idx, uint64_t ntris,
                       const float* quadric_bounds, uint64_t nquadrics, int32_t max_prims_in_node,
                       DrBvhNode* nodes_out, uint64_t* nnodes_out, uint32_t* order_out, uint32_t* depth_out);

/* The same constructor ON THE GPU (dr_bvh_device.hip): identical arguments (host
 * pointers) and byte-identical nodes_out / order_out -- the bounds, the centroid bounds and the 12 SAH buckets are
 * device-wide reductions, the reference's two-pointer `partition` (common.dart:256-287) is the swap of the k-th
 * misplaced item of the left part with the k-th from the end (ranks from one prefix sum), sub-trees of at most 64
 * items are finished by one thread each with the reference's recursion as it stands.  Needs dr_init.  The host
 * builder above stays as the fallback (no GPU) and as this one's checker. */
int dr_bvh_build_device(const float* verts, uint64_t nverts, const uint32_t* tri_idx, uint64_t ntris,
                        const float* quadric_bounds, uint64_t nquadrics, int32_t max_prims_in_node,
                        DrBvhNode* nodes_out, uint64_t* nnodes_out, uint32_t* order_out, uint32_t* depth_out);

/* LoopSubdivision (lib/shapes/loop_subdivision.dart:23-308): the constructor and refine() of Shape "loopsubdiv".
 * indices[nfaces][3] / P[nverts][3]: the control mesh, object space.  Out: the TriangleMesh refine() hands to TriangleMesh.Create -- P_out
 * (the limit positions, object space), N_out (Cross(S, T), object space, not normalised), indices_out[nfaces * 4^nlevels][3] in final face
 * order and final vertex numbering -- bit for bit what the reference's text computes (f32 storage, one f64 operation and one rounding per
 * operator, every sum in one-ring order), with one stated departure: the cos / sin weights of the tangents are the C library's.
 * Two calls, like dr_enumerate_pixels: with P_out, N_out and indices_out all NULL the call validates the mesh and writes only the sizes
 * (*nverts_out, *nfaces_out, always written on DR_OK); with all three set, vert_cap / face_cap are the vertices / faces the buffers hold,
 * too few of either is DR_ERR_INVALID.  nlevels 0 is legal: the limit positions and normals of the control mesh itself.
 * Refused by name (the reference crashes or loops on each): DR_ERR_INVALID for nlevels < 0, a vertex index out of range, a face that repeats
 * a vertex, a vertex that no face names, an edge shared by more than two faces, two faces that traverse a shared edge in the same
 * direction, a vertex whose faces do not form one fan; DR_ERR_UNSUPPORTED for 2^31 or more faces or vertices at the last level.
 * Face order and the rotation of a face's three indices decide startFace and every ring's order, and so the low bits of the output.
 * dr_loop_subdivide runs on the host and needs no GPU. */
int dr_loop_subdivide(const uint32_t* indices, uint64_t nfaces, const float* P, uint64_t nverts, int32_t nlevels, float* P_out,
                      float* N_out, uint32_t* indices_out, uint64_t vert_cap, uint64_t face_cap, uint64_t* nverts_out, uint64_t* nfaces_out);
/* The same ON THE GPU (dr_subdiv_device.hip): identical arguments (host pointers) and byte-identical outputs.  Level 0 -- topology and the
 * refusals -- stays on the host; every level, the limit positions and the normals are kernels over arrays that stay in device memory.
 * Needs dr_init.  The host builder above stays as the fallback (no GPU) and as this one's checker. */
int dr_loop_subdivide_device(const uint32_t* indices, uint64_t nfaces, const float* P, uint64_t nverts, int32_t nlevels, float* P_out,
                             float* N_out, uint32_t* indices_out, uint64_t vert_cap, uint64_t face_cap, uint64_t* nverts_out,
                             uint64_t* nfaces_out);

/* Nurbs (lib/shapes/nurbs.dart:23-321): refine() of Shape "nurbs" -- the patch evaluated at diceu x dicev points
 * and handed to TriangleMesh.Create as one mesh with P, N and uv.  Everything is f32, as the ABI's other geometry: knots, ranges and control
 * points.  cp: nu * nv points, u fastest, 3 floats each ('P', homogeneous 0) or 4 ('Pw', homogeneous 1).  diceu / dicev: points per
 * direction, 0 = the reference's constant 30. */
#define DR_NURBS_MAX_ORDER 8 /* ours: the de Boor work arrays have a fixed size per lane */
typedef struct DrNurbsPatch {
  int32_t nu, uorder;
  const float* uknots; /* nu + uorder */
  float u0, u1;
  int32_t nv, vorder;
  const float* vknots; /* nv + vorder */
  float v0, v1;
  const float* cp;
  int32_t homogeneous;
  uint32_t diceu, dicev;
  uint32_t pad;
} DrNurbsPatch; /* 72 bytes */
/* Out, object space: P_out[nverts][3], N_out[nverts][3] (Normalize(Cross(dPdu, dPdv))), uv_out[nverts][2], indices_out[ntris][3] in the
 * reference's order (:132-142); nverts = diceu * dicev, vertex v * diceu + u, ntris = 2 (diceu - 1)(dicev - 1).  The reference's text
 * with its arithmetic -- f32 stores, f64 expressions in its operator order -- and TWO index expressions repaired: the
 * control point of a work slot is read at cpi + (cpOffset * 4 + i) * cpStride (the text's (cpOffset + i) leaves its iso list beyond the
 * first knot span and raises), and the de Boor step's left operand is cpWork[k + c] (the text's cpWork[j + c] is not the B-spline
 * recurrence from order 3 on).  Bit for bit the reference's output for order 2 x 2 patches of one span; a NURBS surface everywhere.
 * NaN where the arithmetic gives NaN (a zero knot span, a zero weight, a zero cross product); nothing is repaired or skipped there.
 * Two calls, like dr_loop_subdivide: all four outputs NULL validates and writes *nverts / *ntris only; all four set, vert_capacity /
 * tri_capacity are what the buffers hold, too few is DR_ERR_INVALID with nothing written.
 * Refused by name, DR_ERR_INVALID (the evaluation would index outside a list or loop on each): a null patch, knot vector or control net;
 * an order below 2 or above DR_NURBS_MAX_ORDER; nu < uorder or nv < vorder; a knot vector that decreases or holds a non-finite knot;
 * u0 / u1 outside [uknots[uorder - 1], uknots[nu]], v likewise; diceu or dicev below 2 or above 4096, or diceu * dicev above 2^22;
 * nu * nv above 2^24.  dr_nurbs_dice runs on the host and needs no GPU. */
int dr_nurbs_dice(const DrNurbsPatch* patch, float* P_out, float* N_out, float* uv_out, uint32_t* indices_out, uint64_t vert_capacity,
                  uint64_t tri_capacity, uint64_t* nverts, uint64_t* ntris);
/* The same ON THE GPU (dr_nurbs_device.hip): identical arguments (host pointers) and byte-identical outputs, except that a NaN's sign
 * and payload may differ.  One lane per dice point.  Needs dr_init. */
int dr_nurbs_dice_device(const DrNurbsPatch* patch, float* P_out, float* N_out, float* uv_out, uint32_t* indices_out, uint64_t vert_capacity,
                         uint64_t tri_capacity, uint64_t* nverts, uint64_t* ntris);

/* The edge-avoiding a-trous denoiser (the reference has none): a post-process beside the render path, guided by
 * the images of DR_INTEGRATOR_FEATURE.  Row-major f32 images: rgb[h][w][3] (the beauty image), normal[h][w][3] (any 3-vector guide; a
 * DR_FEATURE_NS / _NG image as it stands), depth[h][w] (a scalar guide; channel 0 of a DR_FEATURE_DEPTH image), out[h][w][3].
 * Level i = 0 .. iterations - 1 filters the level before it (level 0: rgb) with the 5 x 5 B3-spline taps at step 2^i; a tap's weight is
 * divided by (1 + k * d) for each of the three squared distances d (colour, normal, depth) whose k is not 0.  k = 1 / sigma^2; the
 * colour term's k is k_color * 4^i at level i.  A pixel with a non-finite colour, normal or depth is copied through bit for bit and is
 * no tap of any other pixel.  f32 arithmetic, one rounding per operator: the three entry points below write the same bytes. */
typedef struct DrDenoiseParams {
  int32_t iterations; /* 1 .. 8 */
  float k_color;      /* finite, >= 0; 0: the term is off.  k_color * 4^(iterations - 1) must be finite in f32 */
  float k_normal;
  float k_depth;
} DrDenoiseParams; /* 16 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer, w or h < 1, w * h >= 2^31, iterations outside 1 .. 8, a k that is negative or not
 * finite, a last level's colour k that is not finite, `out` overlapping an input (or the scratch buffer).
 * dr_denoise_atrous_host: host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_denoise_atrous_host(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h, const DrDenoiseParams* params,
                           float* out);
/* The same ON THE GPU (dr_denoise_device.hip), host buffers: uploads, filters, copies back.  Needs dr_init. */
int dr_denoise_atrous(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h, const DrDenoiseParams* params,
                      float* out);
/* The same on device buffers, asynchronous on the given hipStream_t.  scratch_dev == NULL: the size query -- writes the bytes of scratch
 * an image of w x h needs to *scratch_bytes and does nothing else (the image pointers are not read and may be NULL).  Otherwise
 * *scratch_bytes is the size of scratch_dev (too small is DR_ERR_INVALID), which must be 16-byte aligned and is the call's to overwrite
 * until the stream has run it. */
int dr_denoise_atrous_device(const void* rgb_dev, const void* normal_dev, const void* depth_dev, int32_t w, int32_t h,
                             const DrDenoiseParams* params, void* out_dev, void* scratch_dev, uint64_t* scratch_bytes, void* hip_stream);

/* The variance-guided a-trous denoiser over two half-sample renders: a[h][w][3] and b[h][w][3] are two renders of
 * one scene that differ in the sampler's seed alone, normal and depth the guides above.  Their mean 0.5 * (a + b) is the image that is
 * filtered, and 0.25 * lum(a - b)^2 the first estimate of its luminance variance, which every level carries on (sum of wt^2 * v over
 * (sum of wt)^2) and, smoothed over 3 x 3 pixels, uses as the unit of its colour term: a tap's weight is divided by
 * (1 + k_color * (lum(q) - lum(p))^2 / (variance + var_floor)), with the same k_color at every level, and by the normal and depth terms
 * above.  out[h][w][3]: the filtered mean; out_var[h][w], which may be NULL: its variance, -1 where the pixel is not valid -- a pixel whose
 * mean, first variance, normal or depth is not finite, which is copied through (the mean) and is no tap of any other pixel.  f32
 * arithmetic, one rounding per operator: the three entry points below write the same bytes. */
typedef struct DrDenoisePairParams {
  int32_t iterations; /* 1 .. 8 */
  float k_color;      /* finite, >= 0; 0: the term is off.  1 / sigma^2, sigma in standard deviations of the local noise */
  float k_normal;     /* as in DrDenoiseParams */
  float k_depth;
  float var_floor;    /* finite, > 0: added to the smoothed variance, in squared units of radiance */
} DrDenoisePairParams; /* 20 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer (out_var excepted), w or h < 1, w * h >= 2^31, iterations outside 1 .. 8, a k that is
 * negative or not finite, a var_floor that is not finite or not positive, `out` or `out_var` overlapping an input, each other (or the
 * scratch buffer).
 * dr_denoise_pair_host: host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_denoise_pair_host(const float* a, const float* b, const float* normal, const float* depth, int32_t w, int32_t h,
                         const DrDenoisePairParams* params, float* out, float* out_var);
/* The same ON THE GPU (dr_denoise_device.hip), host buffers: uploads, filters, copies back.  Needs dr_init. */
int dr_denoise_pair(const float* a, const float* b, const float* normal, const float* depth, int32_t w, int32_t h,
                    const DrDenoisePairParams* params, float* out, float* out_var);
/* The same on device buffers, asynchronous on the given hipStream_t; the scratch buffer and its size query as for
 * dr_denoise_atrous_device (the same size). */
int dr_denoise_pair_device(const void* a_dev, const void* b_dev, const void* normal_dev, const void* depth_dev, int32_t w, int32_t h,
                           const DrDenoisePairParams* params, void* out_dev, void* out_var_dev, void* scratch_dev, uint64_t* scratch_bytes,
                           void* hip_stream);

/* The joint bilateral upsampler (Kopf et al. 2007 with the denoiser's rational edge-stopping weights): a beauty image
 * rendered at 1/factor of the resolution per axis, rgb_lo[hl][wl][3], with guides aligned with it, normal_lo[hl][wl][3] and depth_lo[hl][wl],
 * becomes out[h][w][3], w = factor * wl, h = factor * hl, under the full-resolution guides normal[h][w][3] and depth[h][w].  Pixel (x, y) is
 * the weighted mean of the taps x taps low-resolution pixels around (u, v) = ((x + 0.5) / factor - 0.5, (y + 0.5) / factor - 0.5) that lie
 * inside the image and are valid (colour, normal and depth finite); a tap's weight is the tent (1 - |u - i| / r) * (1 - |v - j| / r),
 * r = taps / 2, divided by (1 + k * d) for the squared normal and depth distance between the tap's guide and the pixel's own, each only
 * where its k is not 0 and the pixel's own guide is finite.  No tap, or every weight 0: the colour of low-resolution pixel
 * (x / factor, y / factor), bit for bit.  f32 arithmetic, one rounding per operator: the three entry points below write the same bytes. */
typedef struct DrUpsampleParams {
  int32_t factor;  /* 2 or 4 */
  int32_t taps;    /* 2 or 4: the footprint is taps x taps low-resolution pixels */
  float k_normal;  /* finite, >= 0; 0: the term is off.  As in DrDenoiseParams */
  float k_depth;
} DrUpsampleParams; /* 16 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer, a factor or taps other than 2 or 4, wl or hl < 1, w * h >= 2^31, a k that is negative
 * or not finite, `out` overlapping an input (or the scratch buffer).  dr_upsample_check states them without an image. */
int dr_upsample_check(const DrUpsampleParams* params, int32_t wl, int32_t hl);
/* dr_upsample_host: host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_upsample_host(const float* rgb_lo, const float* normal_lo, const float* depth_lo, int32_t wl, int32_t hl, const float* normal,
                     const float* depth, const DrUpsampleParams* params, float* out);
/* The same ON THE GPU (dr_upsample_device.hip), host buffers: uploads, upsamples, copies back.  Needs dr_init. */
int dr_upsample(const float* rgb_lo, const float* normal_lo, const float* depth_lo, int32_t wl, int32_t hl, const float* normal,
                const float* depth, const DrUpsampleParams* params, float* out);
/* The same on device buffers, asynchronous on the given hipStream_t.  scratch_dev == NULL: the size query -- writes the bytes of scratch a
 * low-resolution image of wl x hl needs to *scratch_bytes and does nothing else (the image pointers are not read and may be NULL).
 * Otherwise *scratch_bytes is the size of scratch_dev (too small is DR_ERR_INVALID), which must be 16-byte aligned and is the call's to
 * overwrite until the stream has run it. */
int dr_upsample_device(const void* rgb_lo_dev, const void* normal_lo_dev, const void* depth_lo_dev, int32_t wl, int32_t hl,
                       const void* normal_dev, const void* depth_dev, const DrUpsampleParams* params, void* out_dev, void* scratch_dev,
                       uint64_t* scratch_bytes, void* hip_stream);

/* Temporal accumulation with reprojection (the temporal half of Schied et al. 2017): the frames of a camera animation
 * share their samples where a surface stays visible.  A call reads the current frame -- rgb[h][w][3], normal[h][w][3] as the feature integrator
 * encodes it and depth[h][w], the ray parameter t along the normalised camera ray -- and the history the previous call left: h_rgb[h][w][3],
 * h_m2[h][w] (the accumulated second moment of the luminance), h_len[h][w] (the history length as f32; 0: none) and the previous frame's
 * guides h_normal / h_depth.  The five history pointers may be NULL together: the first frame.  It writes out_rgb, out_m2 and out_len, the next
 * call's h_rgb, h_m2 and h_len; the current normal and depth are the next call's h_normal and h_depth (the caller hands them over, nothing is
 * copied).  A pixel whose colour, normal and depth are finite and whose depth is > 0 is taken along its camera ray to the point at t (f64),
 * through cur_to_prev to the previous camera's space and through prev_to_raster to the previous raster; (u, v) is rounded to f32 and snapped to
 * 1/256 of a pixel; the 2 x 2 previous pixels around it that lie inside the image, have h_len > 0 and finite values, a depth within
 * depth_tol * tz of the point's distance tz from the previous camera and an encoded normal within normal_tol (squared distance) of the pixel's
 * give the history as their bilinear mean, and out = hist + (cur - hist) / N with N = min(len + 1, max_history).  Every other pixel restarts:
 * out_rgb = rgb bit for bit, out_m2 = lum^2, out_len = 1 (m2 = 0 where lum^2 is not finite, len = 0 where the colour is not).  The matrices are
 * row-major and are not inverted or composed here.  f64 geometry, f32 blending, one rounding per operator: the entry points below write the
 * same bytes. */
typedef struct DrTemporalParams {
  double raster_to_camera[16]; /* the current camera's */
  double cur_to_prev[16];      /* current camera space -> previous camera space; affine: the last row is not read */
  double prev_to_raster[16];   /* previous camera space -> previous raster; projective: rows 0, 1 and 3 are read */
  float depth_tol;             /* relative; finite, >= 0 */
  float normal_tol;            /* squared distance of the encoded normals; finite, >= 0 */
  int32_t max_history;         /* 1..4096: the blend weight never falls below 1 / max_history */
  uint32_t reserved;           /* 0 */
} DrTemporalParams; /* 400 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer other than the all-NULL history, a history that is only partly NULL, w or h < 1,
 * w * h >= 2^31, a tolerance that is negative or not finite, max_history outside 1..4096, a matrix element that is not finite, an output
 * overlapping an input or another output.  dr_temporal_check states those of the parameters and the size without an image. */
int dr_temporal_check(const DrTemporalParams* params, int32_t w, int32_t h);
/* dr_temporal_host: host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_temporal_host(const float* rgb, const float* normal, const float* depth, const float* h_rgb, const float* h_m2, const float* h_len,
                     const float* h_normal, const float* h_depth, int32_t w, int32_t h, const DrTemporalParams* params, float* out_rgb,
                     float* out_m2, float* out_len);
/* The same ON THE GPU (dr_temporal_device.hip), host buffers: uploads, one launch, copies back.  Needs dr_init. */
int dr_temporal(const float* rgb, const float* normal, const float* depth, const float* h_rgb, const float* h_m2, const float* h_len,
                const float* h_normal, const float* h_depth, int32_t w, int32_t h, const DrTemporalParams* params, float* out_rgb, float* out_m2,
                float* out_len);
/* The same on device buffers, asynchronous on the given hipStream_t: one kernel launch.  It needs no scratch buffer, so there is no size
 * query; the parameters are copied at the call and may change as soon as it returns. */
int dr_temporal_device(const void* rgb_dev, const void* normal_dev, const void* depth_dev, const void* h_rgb_dev, const void* h_m2_dev,
                       const void* h_len_dev, const void* h_normal_dev, const void* h_depth_dev, int32_t w, int32_t h,
                       const DrTemporalParams* params, void* out_rgb_dev, void* out_m2_dev, void* out_len_dev, void* hip_stream);

/* Firefly suppression: a guide-aware outlier clamp that runs ahead of the filters and of the temporal history.
 * rgb[h][w][3], normal[h][w][3] and depth[h][w] are the images of dr_temporal*.  A pixel is valid where its three colour values, three normal
 * values and depth are finite and its luminance L is finite.  The members of a valid pixel p are the valid pixels q != p of its
 * (2 radius + 1)^2 window inside the image with |z_q - z_p| <= depth_tol * z_p and a squared distance of the encoded normals <= normal_tol
 * (dr_temporal*'s agreement test).  With n members, n >= rank, m the rank-th largest member luminance, T = threshold * m + floor and
 * T0 = T > 0 ? T : 0: where L > T0 the colour is scaled by T0 / L; every other pixel -- invalid, n < rank, or not brighter -- is copied bit
 * for bit.  out[h][w][3]: the result; removed[h][w], which may be NULL: L - T0 where the pixel was scaled and 0 elsewhere.  The taps read
 * the original image, so the stage cannot run in place.  f32 arithmetic, one rounding per operator: the entry points below write the same
 * bytes. */
typedef struct DrFireflyParams {
  int32_t radius;   /* 1 or 2: the window is (2 radius + 1)^2 pixels */
  int32_t rank;     /* 1..4: the member luminance the limit is taken from, counted from the largest */
  float threshold;  /* finite, >= 0 */
  float floor;      /* finite, not < 0: added to the limit, in radiance */
  float depth_tol;  /* as in DrTemporalParams */
  float normal_tol; /* as in DrTemporalParams */
} DrFireflyParams; /* 24 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer (removed excepted), w or h < 1, w * h >= 2^31, radius other than 1 or 2, rank outside
 * 1..4, a threshold, floor or tolerance that is negative or not finite, out or removed overlapping an input or each other.
 * dr_firefly_check states those of the parameters and the size without an image. */
int dr_firefly_check(const DrFireflyParams* params, int32_t w, int32_t h);
/* dr_firefly_host: host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_firefly_host(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h, const DrFireflyParams* params, float* out,
                    float* removed);
/* The same ON THE GPU (dr_firefly_device.hip), host buffers: uploads, one launch, copies back.  Needs dr_init. */
int dr_firefly(const float* rgb, const float* normal, const float* depth, int32_t w, int32_t h, const DrFireflyParams* params, float* out,
               float* removed);
/* The same on device buffers, asynchronous on the given hipStream_t: one kernel launch.  It needs no scratch buffer, so there is no size
 * query; the parameters are copied at the call and may change as soon as it returns. */
int dr_firefly_device(const void* rgb_dev, const void* normal_dev, const void* depth_dev, int32_t w, int32_t h, const DrFireflyParams* params,
                      void* out_dev, void* removed_dev, void* hip_stream);

/* Demodulation: what is known per sample without noise is taken out of the beauty image before any other image stage
 * and put back after the last.  rgb[h][w][3] is the beauty image; emission[h][w][3] and albedo[h][w][3] are the images of
 * DR_INTEGRATOR_MATERIAL, and either may be NULL: an absent emission is 0, an absent albedo makes the divisor 1.  Per pixel and colour
 * channel, f32 with one rounding per operator:
 *   dr_demodulate*:  out = max(0, rgb - e) / (a + eps)        (the subtraction's result where it is > 0, else 0.0f)
 *   dr_remodulate*:  out = f * (a + eps) + e                  (rgb is the filtered, demodulated image f)
 * A pixel with a value of rgb, emission or albedo that is not finite is copied from rgb bit for bit by both.  out must not overlap an
 * input.  The entry points of one operation write the same bytes. */
typedef struct DrDemodulateParams {
  float eps; /* finite, > 0: added to the albedo, so that a black surface divides by eps and not by 0 */
} DrDemodulateParams; /* 4 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer (emission and albedo excepted), w or h < 1, w * h >= 2^31, an eps that is not
 * finite or not positive, out overlapping an input.  dr_demodulate_check states those of the parameters and the size without an image. */
int dr_demodulate_check(const DrDemodulateParams* params, int32_t w, int32_t h);
/* Host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_demodulate_host(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h, const DrDemodulateParams* params,
                       float* out);
int dr_remodulate_host(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h, const DrDemodulateParams* params,
                       float* out);
/* The same ON THE GPU (dr_demodulate_device.hip), host buffers: uploads, one launch, copies back.  Needs dr_init. */
int dr_demodulate(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h, const DrDemodulateParams* params, float* out);
int dr_remodulate(const float* rgb, const float* emission, const float* albedo, int32_t w, int32_t h, const DrDemodulateParams* params, float* out);
/* The same on device buffers, asynchronous on the given hipStream_t: one kernel launch (k_demodulate / k_remodulate), no scratch buffer and
 * no size query, as for dr_firefly_device; the parameters are copied at the call. */
int dr_demodulate_device(const void* rgb_dev, const void* emission_dev, const void* albedo_dev, int32_t w, int32_t h,
                         const DrDemodulateParams* params, void* out_dev, void* hip_stream);
int dr_remodulate_device(const void* rgb_dev, const void* emission_dev, const void* albedo_dev, int32_t w, int32_t h,
                         const DrDemodulateParams* params, void* out_dev, void* hip_stream);

/* The variance-guided a-trous denoiser over a temporal history (the variance estimate of Schied et al. 2017,
 * section 4.2, in front of the levels of section 2.19): rgb[h][w][3], m2[h][w] and len[h][w] are what dr_temporal* wrote last -- the
 * accumulated colour, the accumulated second moment of its luminance and the history length -- and normal and depth that frame's guides.
 * A pixel is valid where all nine values are finite and len > 0.  Its first variance is, with l = lum(rgb): where len >= min_history,
 * max(0, m2 - l * l) / (len - 1), the sample variance of the per-frame luminance taken as the variance of the accumulated mean; where
 * the history is shorter, max(0, s2 / sw - (s1 / sw)^2) over the valid pixels q of the (2 radius + 1)^2 window inside the image, with
 * s1, s2 and sw the sums of wt * lum(q), wt * lum(q)^2 and wt, and wt = 1 divided by the normal and depth terms of DrDenoiseParams.  A
 * first variance that is not finite makes the pixel invalid.  The levels are those of dr_denoise_pair* on (rgb, first variance).
 * out[h][w][3]: the filtered colour; out_var[h][w], which may be NULL: its variance after the last level; out_var0[h][w], which may be
 * NULL: the first variance, before any level; both -1 where the pixel is not valid -- such a pixel is copied through and is no tap of
 * any other pixel.  f32 arithmetic, one rounding per operator: the three entry points below write the same bytes. */
typedef struct DrDenoiseMomentsParams {
  int32_t iterations;  /* 1 .. 8 */
  float k_color;       /* as in DrDenoisePairParams */
  float k_normal;      /* as in DrDenoiseParams; also the spatial estimate's */
  float k_depth;
  float var_floor;     /* as in DrDenoisePairParams */
  int32_t min_history; /* 2 .. 4096: a history of at least this many frames gives the temporal estimate */
  int32_t radius;      /* 0 .. 3: the spatial estimate's window is (2 radius + 1)^2 pixels */
} DrDenoiseMomentsParams; /* 28 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer (out_var and out_var0 excepted), w or h < 1, w * h >= 2^31, iterations outside
 * 1 .. 8, a k that is negative or not finite, a var_floor that is not finite or not positive, min_history outside 2 .. 4096, radius
 * outside 0 .. 3, an output overlapping an input, another output (or the scratch buffer).  dr_denoise_moments_check states those of
 * the parameters and the size without an image. */
int dr_denoise_moments_check(const DrDenoiseMomentsParams* params, int32_t w, int32_t h);
/* dr_denoise_moments_host: host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_denoise_moments_host(const float* rgb, const float* m2, const float* len, const float* normal, const float* depth, int32_t w,
                            int32_t h, const DrDenoiseMomentsParams* params, float* out, float* out_var, float* out_var0);
/* The same ON THE GPU (dr_denoise_device.hip), host buffers: uploads, filters, copies back.  Needs dr_init. */
int dr_denoise_moments(const float* rgb, const float* m2, const float* len, const float* normal, const float* depth, int32_t w, int32_t h,
                       const DrDenoiseMomentsParams* params, float* out, float* out_var, float* out_var0);
/* The same on device buffers, asynchronous on the given hipStream_t; the scratch buffer and its size query as for
 * dr_denoise_pair_device (the same size). */
int dr_denoise_moments_device(const void* rgb_dev, const void* m2_dev, const void* len_dev, const void* normal_dev, const void* depth_dev,
                              int32_t w, int32_t h, const DrDenoiseMomentsParams* params, void* out_dev, void* out_var_dev,
                              void* out_var0_dev, void* scratch_dev, uint64_t* scratch_bytes, void* hip_stream);

/* The display transform: rgb[h][w][3], row-major f32 linear radiance, becomes out[h][w][4], bytes R, G, B, A = 255.
 * Per pixel: a non-finite channel makes the pixel invalid (it is no sample of the histogram and comes out as invalid_rgba); a negative channel
 * is taken as 0; the channels are multiplied by the exposure scale, go through the tone curve and are encoded to a byte each.  The scale is
 * `exposure`, or with auto_exposure != 0 key over the centre of the luminance-histogram bin (2048 bins, eight per octave: the f32's bits
 * >> 20) in which the pixel of rank (n - 1) * permille / 1000 among the n counted ones lies; 1 when none is counted.  f32 arithmetic, one
 * rounding per operator, no transcendental per pixel: the entry points below write the same bytes. */
#define DR_TONE_CLAMP 0u       /* identity */
#define DR_TONE_REINHARD 1u    /* Yd = (Y * (1 + Y * inv_white2)) / (1 + Y) on the luminance Y; the colour is scaled by Yd / Y */
#define DR_TONE_FILMIC 2u      /* (x * (2.51 x + 0.03)) / (x * (2.43 x + 0.59) + 0.14) per channel */
#define DR_ENCODE_SRGB 0u      /* the number of thresholds T[1..255] <= x; T[k] is the linear value that the sRGB curve takes to (k - 0.5) / 255 */
#define DR_ENCODE_GAMMA22 1u   /* the same with T[k] = ((k - 0.5) / 255)^2.2 */
#define DR_ENCODE_REFERENCE 2u /* ImageFilm's: G[clamp(floor(f64(x) * 255.0), 0, 255)], G[i] = clamp(floor(pow(i / 255.0, 1.0 / 2.2) * 255.0), 0, 255) */
#define DR_DISPLAY_BINS 2048u
typedef struct DrDisplayParams {
  uint32_t curve;         /* DR_TONE_* */
  uint32_t encode;        /* DR_ENCODE_* */
  uint32_t auto_exposure; /* 0: the scale is `exposure`; else it is found from the histogram */
  uint32_t permille;      /* 0 .. 1000; 500 is the median */
  float exposure;         /* finite, > 0 */
  float key;              /* finite, > 0; the value the picked luminance is mapped to (0.18: middle grey) */
  float inv_white2;       /* finite, >= 0: 1 / white^2 of the extended Reinhard curve; 0 is the plain Y / (1 + Y) */
  uint32_t invalid_rgba;  /* r | g << 8 | b << 16 | a << 24 of an invalid pixel (0xff000000: opaque black) */
} DrDisplayParams; /* 32 bytes */
/* Refused with DR_ERR_INVALID, by name: a null pointer, an unknown curve or encode, permille > 1000, an exposure or key that is not finite or
 * not positive, an inv_white2 that is negative or not finite, w or h < 1, w * h >= 2^31, `out` overlapping `rgb` (or the scratch buffer).
 * dr_display_check states them without an image. */
int dr_display_check(const DrDisplayParams* params, int32_t w, int32_t h);
/* The 256 words of an encode's table: for DR_ENCODE_SRGB and _GAMMA22 word 0 is 0 and word k the f32 T[k]; for DR_ENCODE_REFERENCE word i
 * is G[i].  Computed in f64 with the C library's pow; every entry point reads this table.  n, the words `out` has room for, must be 256. */
int dr_display_table(uint32_t encode, uint32_t* out, uint32_t n);
/* dr_display_host: host buffers, a serial loop, no GPU needed -- the fallback and the device version's checker. */
int dr_display_host(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, uint8_t* out);
/* The same ON THE GPU (dr_display_device.hip), host buffers: uploads, transforms, copies back.  Needs dr_init. */
int dr_display(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, uint8_t* out);
/* The same on device buffers, asynchronous on the given hipStream_t, with no wait on the host between the histogram and the encode.
 * scratch_dev == NULL: the size query -- writes the bytes of scratch a call needs to *scratch_bytes and does nothing else (the image pointers
 * are not read and may be NULL).  Otherwise *scratch_bytes is the size of scratch_dev (too small is DR_ERR_INVALID), which must be 16-byte
 * aligned and is the call's to overwrite until the stream has run it: the 2048 counts, then the scale. */
int dr_display_device(const void* rgb_dev, int32_t w, int32_t h, const DrDisplayParams* params, void* out_dev, void* scratch_dev,
                      uint64_t* scratch_bytes, void* hip_stream);
/* The scale auto-exposure picks for this image with params' key and permille (auto_exposure itself is not read), to *scale, and the 2048
 * counts to hist unless it is NULL.  dr_display_exposure_host: no GPU needed; dr_display_exposure: on the GPU, host buffers, needs dr_init. */
int dr_display_exposure_host(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, float* scale, uint32_t* hist);
int dr_display_exposure(const float* rgb, int32_t w, int32_t h, const DrDisplayParams* params, float* scale, uint32_t* hist);

/* Scene upload (replaces the construction of lib/core/scene.dart Scene). */
int dr_scene_create(const DrSceneDesc* desc, DrScene** out);
void dr_scene_destroy(DrScene* scene);

/* Which traversal kernel each ray kind ([0] closest hit, [1] any hit) uses on this scene: 0 = not decided yet (the
 * first big render of a big scene measures the candidates on calibration batches of its own samples, rendered into the
 * film like any other: DrRenderStats.pilot_ms), 2 = one node per step, 3 = sibling pairs, 5 (closest-hit rays only) =
 * sibling pairs with the ray's cold state in LDS, six workgroups per CU.  All are bit-exact; only speed depends on the choice.  A host that renders the same
 * scene again (another frame, another process) can store the measured choice and hand it back: the pilot is then
 * skipped.  Setting 0 makes the next big render measure again. */
int dr_scene_get_trace_kernels(const DrScene* scene, uint32_t kernels_out[2]);
int dr_scene_set_trace_kernels(DrScene* scene, const uint32_t kernels[2]);
/* What the pilot measured, in ms per algorithmic GB (32 B per node visit + 48 B per triangle test of the calibration
 * batch's own counters): out[0..2] closest-hit rays with kernel 2 / 3 / 5, out[3..4] any-hit rays with kernel 2 / 3,
 * out[5] reserved (0).  0 = not measured (no pilot has run, the kernels were set by the host, or that candidate was
 * skipped: kernel 5 is not timed where kernel 3 lost to kernel 2 by more than 5 %).  Diagnostics: how close a choice was. */
int dr_scene_get_pilot(const DrScene* scene, float ms_per_gb_out[6]);
/* Diagnostics: what the scene's LAST dr_render_device call actually ran with, switches (dr_set_option / environment)
 * included -- out[0] path-state layout (64 / 4), out[1] / out[2] the traversal kernel of its closest-hit / any-hit launches
 * (2, 3, 5 as above), out[3] -1, or after a DR_INTEGRATOR_WHITTED, DR_INTEGRATOR_AO, DR_INTEGRATOR_FEATURE, DR_INTEGRATOR_MATERIAL or DR_INTEGRATOR_DIFFUSE_PRT render the integrator and its shading
 * kernels: bits 0-7 the DR_INTEGRATOR_* constant, bit 8 k_shade_whitted ran, bit 9 k_shade_spec ran (the scene has mirror / glass), bit 10
 * k_shade_ao ran, bit 11 k_shade_feature ran (bits 12-14: its DR_FEATURE_* channel), bit 15 k_shade_prt ran, bit 16 k_shade_gprt and k_gprt_finish
 * ran (DR_INTEGRATOR_GLOSSY_PRT), bit 17 k_shade_probes ran, bit 18 k_shade_material ran (bit 19: its DR_MATERIAL_CHANNEL_* channel); out[4] the
 * calibration batches it ran (0: no pilot), out[5] its batches, out[6] workgroups per CU of a persistent traversal
 * launch, out[7] bit 0: a stage's any-hit launch ran beside its closest-hit launch, bit 1: the camera rays went through the
 * wave-coherent kernel (k_trace_pk), bit 3: the device sampler generated bounce b's blocks only for the pixel
 * groups alive at bounce b (DARTRAY_LAZY_GEN).  All 0 / -1 before the first render. */
int dr_scene_last_render_info(const DrScene* scene, int32_t info_out[8]);
/* Diagnostics: the part of DrRenderStats' closest-hit totals (closest_rays / _nodes / _tris / _launches / _ms, accumulated since the last
 * dr_reset_stats) that the wave-coherent kernel k_trace_pk traced -- the camera rays -- as out[0] rays, out[1] node visits, out[2]
 * triangle tests, out[3] launches, out[4] ms.  Waits for the renders in flight like dr_get_stats.  What is left after subtracting them
 * belongs to the per-lane closest-hit kernel (k_trace<0> / k_trace3<0> / k_trace3c): how bench.py prices the two separately. */
int dr_scene_get_coherent_stats(DrScene* scene, double out[5]);
/* Diagnostics: the device sampler's work since the last dr_reset_stats, in (pixel, LD block) pairs -- one pair = one shuffled run of
 * spp indices.  out[0]: pairs generated; out[1]: pairs the integrator's reads name (every block a path of maximal length would read,
 * for every pixel).  Equal unless generation is lazy (DARTRAY_LAZY_GEN, the default for path renders at >= 64 spp) and paths end
 * early: bounce b's blocks are shuffled only for 64-pixel groups with a path alive at bounce b.  Both 0 for the host-buffer sampler
 * and the full-float sample form.  Waits for the renders in flight like dr_get_stats. */
int dr_scene_get_sampler_stats(DrScene* scene, double out[2]);
/* Device memory the scene's path-state workspace holds right now (tiles, queues, sample storage; it is allocated by the first render,
 * grows when a later render needs more and is freed with the scene): what a host budgets next to its own allocations. */
int dr_scene_workspace_bytes(const DrScene* scene, uint64_t* bytes_out);
/* Diagnostics: what the shading kernels' light and material tables of this scene hold -- out[0] light records, out[1] light-triangle
 * records (a quadric emitter counts one), out[2] entries of the lights' area CDFs (triangles + 1 per area light; 1 where there is none),
 * out[3] material records, out[4] / out[5] the bytes of one light / one light-triangle record.  Their byte sizes decide per scene whether
 * the shading kernels read the tables from LDS or from global memory ("Where the tables live"): results never
 * depend on it, and a test that means to cover one side says so with these counts. */
int dr_scene_get_table_counts(const DrScene* scene, uint32_t counts_out[6]);
/* The path-state layout of this scene's path-traced renders, next to the traversal kernels and measured the same way: the
 * first big render's first pilot batch counts how many of its slots are still alive at the second bounce (density_out;
 * -1 before); below one half the renders use four-slot, line-grouped sub-tiles (layout 4: stage lists that thin out touch
 * few lines per surviving slot), otherwise 64-slot runs (layout 64).  Results never depend on it.  A host can store the
 * choice with the scene and hand it back (0 = measure again at the next big render). */
int dr_scene_get_state_layout(const DrScene* scene, int32_t* layout_out, float* density_out);
/* Diagnostics: what dr_scene_create derived from the marshalled tree -- the sibling-pair records of the v3 traversal kernels
 * (64 bytes each: the two child nodes of an interior node side by side, a child's `offset` naming its own pair record; 0 records
 * when the tree cannot use them), how many of them form the breadth-first top of the tree, and the height it measured.  out may
 * be NULL to query the counts. */
int dr_scene_get_pairs(const DrScene* scene, void* out, uint64_t cap_bytes, uint64_t* npairs_out, uint32_t* top_pairs_out, uint32_t* depth_out);
int dr_scene_set_state_layout(DrScene* scene, int32_t layout);

/* Aggregate.intersect / Aggregate.intersectP (lib/core/primitive.dart:33-55 ->
 * bvh_accel.dart:101-226) on a batch of rays; host buffers. */
int dr_intersect(DrScene* scene, const DrRay* rays, int64_t n, DrHit* out, int32_t any_hit);

/* Floats per camera-sample vector for an integrator (Sample layout,
 * lib/core/sample.dart:23-79). */
int32_t dr_sample_floats(int32_t integrator, uint32_t nlights);
/* Same for an uploaded scene: DirectLighting requests roundSize(light.nSamples) entries per light slot
 * (direct_lighting_integrator.dart:70-87; low_discrepancy_sampler.dart:43-49), so the vector length depends on
 * the lights; dr_sample_floats assumes nsamples == 1 everywhere. */
int32_t dr_scene_sample_floats(const DrScene* scene, int32_t integrator);
/* What a DR_INTEGRATOR_FEATURE render of `channel` over a scene of `nprimitives` primitives would answer, without a scene or a device: DR_OK,
 * DR_ERR_INVALID (no such channel) or DR_ERR_UNSUPPORTED (DR_FEATURE_ID with 2^24 primitives or more: an index would no longer be exact in the
 * film's f32), with dr_last_error's text.  dr_render* apply the same rule to their scene. */
int dr_feature_check(int32_t channel, uint64_t nprimitives);
/* What a DR_INTEGRATOR_MATERIAL render of `channel` would answer, without a scene or a device: DR_OK, or DR_ERR_INVALID (no such channel)
 * with dr_last_error's text.  dr_render* apply the same rule. */
int dr_material_check(int32_t channel);
/* DiffusePRTIntegrator.preprocess on the device: the scene's incident-light coefficients c_in for `lmax`, after
 * ReduceRinging, as out[(lmax + 1)^2][3] (RGB) -- what a DR_INTEGRATOR_DIFFUSE_PRT render of the scene uses (computed once per scene and lmax).
 * shutter_open is the reference's sample time; no light of the device path reads it.  lmax below 1 or above 8: DR_ERR_INVALID. */
int dr_prt_incident(DrScene* scene, int32_t lmax, double shutter_open, float* out);
/* SphericalHarmonics.Evaluate on the host, as the device evaluates it (one header compiled for both): the (lmax + 1)^2 harmonics of each of
 * the n unit directions dirs[n][3] into out[n][(lmax + 1)^2], f64.  Needs no device.  lmax below 1 or above 8: DR_ERR_INVALID. */
int dr_sh_evaluate(const double* dirs, int64_t n, int32_t lmax, double* out);
/* GlossyPRTIntegrator's Kd, Ks and roughness.  roughness is a Dart double (1 / 0.1 is 10, 1 / 0.1f is not), so it
 * travels as one. */
typedef struct DrGlossyPrtParams {
  float Kd[3];       /* reference default 0.5 */
  float Ks[3];       /* reference default 0.25 */
  double roughness;  /* reference default 0.1 */
} DrGlossyPrtParams;
/* Sets the scene's glossy PRT parameters (the reference's defaults until the first call).  The BSDF matrix is computed at the next
 * DR_INTEGRATOR_GLOSSY_PRT render or dr_prt_bsdf_matrix call and kept per (lmax, nsamples_b, Kd, Ks, roughness).  Nothing is validated, as in
 * the reference: negative or NaN colours go into the matrix as they are; the Blinn exponent 1 / roughness is clamped to 10000 when it is above
 * that or NaN (blinn.dart:24-28), so roughness 0 means 10000 and a negative roughness a negative exponent. */
int dr_scene_set_glossy_prt(DrScene* scene, const DrGlossyPrtParams* params);
/* ComputeBSDFMatrix on the device with nsamples_b directions (a render always uses 1024; 1 .. 1024 here), out[(lmax + 1)^2][(lmax + 1)^2][3].
 * Its scramble is the two draws of the preprocess RNG behind the lights' projection.  lmax below 1 or above 4: DR_ERR_INVALID. */
int dr_prt_bsdf_matrix(DrScene* scene, int32_t lmax, int32_t nsamples_b, float* out);
/* Host builds of the headers the device compiles.  Need no device.
 * dr_sh_rotate: SphericalHarmonics.Rotate of c_in[(lmax + 1)^2][3] by the Matrix4x4 m16 (row major) into out, object sharing included.
 * dr_sh_bsdf_matrix_host: ComputeBSDFMatrix with the given scramble words.  dr_sh_rotate_device: dr_sh_rotate of nframes (c_in, m16) pairs, one
 * device lane per frame and channel. */
int dr_sh_rotate(const float* c_in, const float* m16, int32_t lmax, float* out);
int dr_sh_bsdf_matrix_host(const float* Kd, const float* Ks, double roughness, const uint32_t* scramble, int32_t nsamples_b, int32_t lmax, float* out);
int dr_sh_rotate_device(const float* c_in, const float* m16, int32_t lmax, int32_t nframes, float* out);

/* Radiance probes: CreateProbesRenderer's bake of shadowed direct light onto a 3-D grid of spherical-harmonic probes
 * (renderers/create_probes_renderer.dart), on the device, in stages that can each be called alone. */
typedef struct DrProbesDesc {
  int32_t lmax;             /* 1 .. 8 (reference default 4) */
  int32_t include_indirect; /* must be 0: `indirectlighting` (a full render per probe) is refused by name.  The reference's default is true */
  int32_t npoints;          /* surface points of the visibility test; the reference's constant is 32768 */
  int32_t has_bounds;       /* 0: `bounds` is scene.worldBound */
  float bounds[6];          /* x0 y0 z0 x1 y1 z1 */
  float camera_pos[3];      /* camera.cameraToWorld(shutterOpen, Point.ZERO): where the random walks start */
  float pad;
  double spacing;           /* samplespacing (reference default 1.0) */
  double time;              /* (reference default 0.0; no shape of the device path moves) */
} DrProbesDesc;
/* Stage 1 (:78-121): the points the random walks from camera_pos deposit -- the camera position, then per walk up to 32 closest hits against the
 * scene or, where it misses, the bounding sphere of its world bound -- on one RNG(5489) stream.  out: room for npoints + 31 points (the
 * inner loop does not re-check the length); *count_out: how many were written. */
int dr_probes_surface_points(DrScene* scene, const float camera_pos[3], double time, int32_t npoints, float* out, int32_t* count_out);
/* nProbes[i] = max(1, ceil(delta[i] / spacing)) and the bounds the desc means (lmax and npoints are not read). */
int dr_probes_grid(const DrScene* scene, const DrProbesDesc* desc, int32_t nprobes_out[3], float bounds_out[6]);
/* Stage 2 (:254-309): per cell the first 32 of its 256 candidates, in index order, that some of the given points sees:
 * nfound_out[cells], accepted_out[cells][32] (candidate indices, -1 behind the last).  desc: bounds and spacing. */
int dr_probes_candidates(DrScene* scene, const DrProbesDesc* desc, const float* points, int32_t npoints, int32_t* nfound_out, int32_t* accepted_out);
/* Stages 1 to 3: the reference's Float32List -- lmax, includeDirect (1), includeIndirect (0), nProbes[3], the six bounds, the coefficients
 * [cell][(lmax + 1)^2][3], three zeros -- into out[nfloats], nfloats = 15 + cells * (lmax + 1)^2 * 3 exactly (dr_probes_grid gives the cells). */
int dr_probes_bake(DrScene* scene, const DrProbesDesc* desc, float* out, int64_t nfloats);
/* Attaches a probe grid in that form to the scene for DR_INTEGRATOR_USE_PROBES renders (a copy is kept on the device); data NULL detaches it.
 * The header is checked against n: lmax in 1 .. 8, nProbes whole numbers in 1 .. 4096, n = 15 + cells * (lmax + 1)^2 * 3, else DR_ERR_INVALID. */
int dr_scene_set_probes(DrScene* scene, const float* data, int64_t n);

/* Renderer.render(Scene) (lib/core/renderer.dart:28;
 * sampler_renderer.dart:36-65): traces this task's window and returns the
 * film.  film_out: [height*width*4] f32 (X, Y, Z, weightSum) -- ImageFilm's
 * _Lxyz/_weightSum (image_film.dart:69-71); rgb_out (optional):
 * [height*width*3] = OutputImage.rgb after ImageFilm.writeImage (:268-299). */
int dr_render(DrScene* scene, const DrRenderDesc* desc, float* film_out, float* rgb_out);

/* Same, with the film left in device memory (accumulated into film_dev, which
 * the caller zero-initialises) on the given hipStream_t; used by bench.py and
 * by the multi-GPU path, which reduces film_dev over RCCL before resolving.
 * Everything the call enqueues is ordered behind earlier work of hip_stream and
 * in front of later work of it; internally a stage's any-hit launch runs on a
 * stream of the scene's own, beside the closest-hit launch, tied to hip_stream
 * by events (DARTRAY_OVERLAP_ANY=0: everything on hip_stream).
 * The call returns with its kernels enqueued, except in four cases where it waits for hip_stream itself: the
 * first big render of a big scene (the traversal-kernel pilot reads its counters back between its three batches),
 * DR_SAMPLER_HOST_BUFFER (the host sample buffers of a batch are staged before the next batch reuses the area),
 * DirectLighting over mirror / glass materials (one count is read back per round of the specular recursion), and
 * DR_SAMPLER_HALTON (per batch, the number of samples its index range accepted is read back before the batch is launched;
 * DR_SAMPLER_ADAPTIVE likewise reads one count between its passes). */
int dr_render_device(DrScene* scene, const DrRenderDesc* desc, void* film_dev, void* hip_stream);

/* Guide images in the beauty render's own pass.  Behind the camera rays' traversal a batch holds every sample's hit record
 * and camera ray -- all a DR_INTEGRATOR_FEATURE render reads -- so one more launch per batch (k_guides) writes the requested DR_FEATURE_* channels'
 * values to side planes, and the batch's film step adds each plane to a film of the channel's own with the beauty film's samples, filter and
 * window.  A channel's film equals the film of a DR_INTEGRATOR_FEATURE render of that channel with the same camera, film, sampler and work split
 * (bit for bit wherever two such renders equal each other: a filter that stays inside the pixel and a pixel-bound sampler); the beauty film
 * equals dr_render's.  Under DirectLighting over mirror / glass the guide is the first hit, as under the feature integrator. */
#define DR_GUIDES_MAX 5
typedef struct DrGuidesDesc {
  int32_t count;                   /* 1 .. DR_GUIDES_MAX */
  int32_t channels[DR_GUIDES_MAX]; /* DR_FEATURE_* values, each at most once; entries behind `count` are not read */
} DrGuidesDesc;
/* What dr_render_guides* would answer to `desc` and `guides` over a scene of `nprimitives` primitives, without a scene or a device: DR_OK, or the
 * refusal with dr_last_error's text.  Served: DR_INTEGRATOR_PATH, _DIRECT_ALL, _DIRECT_ONE, _WHITTED and _AO under every sampler mode the feature
 * integrator accepts.  DR_ERR_UNSUPPORTED, by name: DR_INTEGRATOR_FEATURE, _DIFFUSE_PRT, _GLOSSY_PRT, _USE_PROBES; DR_SAMPLER_ADAPTIVE;
 * DR_FEATURE_ID with 2^24 primitives or more.  DR_ERR_INVALID: an unknown integrator, an empty list, more than DR_GUIDES_MAX channels, an unknown
 * channel, a channel given twice.  Only desc->integrator and desc->sampler_mode are read: everything else of `desc` is checked by the render. */
int dr_render_guides_check(const DrRenderDesc* desc, const DrGuidesDesc* guides, uint64_t nprimitives);
/* dr_render plus the guides: guide_films_out[i] is channel i's film [height*width*4], guide_rgbs_out (optional, as are its entries) channel i's
 * resolved image [height*width*3].  There is no sharded form; task_* and tile_* work as for dr_render. */
int dr_render_guides(DrScene* scene, const DrRenderDesc* desc, const DrGuidesDesc* guides, float* film_out, float* rgb_out,
                     float* const* guide_films_out, float* const* guide_rgbs_out);
/* dr_render_device's twin: the beauty film accumulates into film_dev and channel i's into guide_films_dev[i] (device addresses in a host array;
 * the caller zero-initialises every film), with dr_render_device's stream-ordering contract and its waits. */
int dr_render_guides_device(DrScene* scene, const DrRenderDesc* desc, const DrGuidesDesc* guides, void* film_dev, void* const* guide_films_dev,
                            void* hip_stream);

/* The raster pixels a DR_SAMPLER_COUNTER render of `desc` traces, in trace
 * order (GetSubWindow rectangle, common.dart:52-73, intersected with this
 * rank's round-robin tiles).  Host-only; out_xy may be NULL to query the count. */
int dr_enumerate_pixels(const DrRenderDesc* desc, int32_t* out_xy, uint64_t cap, uint64_t* n_out);

/* Diagnostics and tests: runs ONLY the device sampler of `desc` (DR_SAMPLER_COUNTER, DR_SAMPLER_STRATIFIED* or DR_SAMPLER_RANDOM) for the npix raster
 * pixels pixel_xy[npix][2] -- the launches a render of those pixels makes, into the render's own workspace -- and copies the camera-sample
 * vectors back: out[npix * spp][stride] in reference field order (imageU, imageV, lensU, lensV, time, oneD..., twoD...; the image
 * sample as its fraction inside the pixel), stride >= dr_scene_sample_floats.  Every LD block is produced (a render may skip blocks no
 * kernel reads).  The film window, the task / tile split and the seed of `desc` are read as a render reads them: the streams are keyed by
 * a pixel's position in the full sampler extent. */
int dr_generate_samples(DrScene* scene, const DrRenderDesc* desc, const int32_t* pixel_xy, uint64_t npix, float* out, int32_t stride);

/* Diagnostics and tests: runs ONLY the device sampler of `desc` (DR_SAMPLER_HALTON; any other mode is DR_ERR_INVALID, as this mode is for
 * dr_generate_samples) for the indices [first_index, first_index + count) of the task's sequence -- the selection and generation launches of a
 * render, in the render's own workspace -- and copies back, for the *n_out <= count accepted samples in increasing index order: k_out[n] their
 * indices, pixel_xy_out[n][2] their anchor pixels (floor(imageX), floor(imageY)) and out[n][stride] their sample vectors in reference field order
 * (the image sample as its fraction behind the anchor pixel, time raw), stride >= dr_scene_sample_floats.  The caller sizes the three buffers for
 * `count` entries.  A range that leaves [0, spp * delta * delta) is DR_ERR_INVALID. */
int dr_generate_halton_samples(DrScene* scene, const DrRenderDesc* desc, uint64_t first_index, uint64_t count, uint64_t* k_out,
                               int32_t* pixel_xy_out, float* out, int32_t stride, uint64_t* n_out);

/* Diagnostics and tests: the raster pixels the scene's LAST render call supersampled (DR_SAMPLER_ADAPTIVE: those traced at maxSamples;
 * any other sampler: none), out_xy[n][2] in no particular order.  *n_out is always written; out_xy may be NULL to query the count,
 * cap < n with out_xy set is DR_ERR_INVALID. */
int dr_scene_get_adaptive_pixels(DrScene* scene, int32_t* out_xy, uint64_t cap, uint64_t* n_out);

/* ImageFilm.writeImage on a device film: XYZ -> RGB, divide by weightSum. */
int dr_film_resolve_device(const void* film_dev, int64_t npixels, void* rgb_dev, void* hip_stream);

/* Accumulated stats of this scene (synchronises with the last render's stream work). */
int dr_get_stats(DrScene* scene, DrRenderStats* out);
int dr_reset_stats(DrScene* scene);

/* Device float4 copy kernel: the measured HBM-bandwidth denominator. Returns GB/s. */
int dr_copy_bandwidth(uint64_t bytes, int32_t iters, double* gbps_out);

/* ---- multi-GPU: one process per GPU, the film merged over RCCL -------------------------------------------
 * The reference fans a render out over isolates, one sub-window each, and merges their rectangles in the
 * host (lib/dartray_web/render_manager.dart:100-141; GetSubWindow lib/core/common.dart:52-73).  Here every
 * rank renders its tile share (DrRenderDesc.tile_*) into a zero-initialised full-frame device film with
 * dr_render_device, and ONE ncclReduce(sum, f32) over xGMI merges the films on `root`.  The host only has to
 * carry DR_COMM_ID_BYTES from rank 0 to the other ranks (any channel: a file, a socket, MPI, torchrun's
 * store).  librccl is loaded on the first dr_comm_* call (DARTRAY_RCCL_LIB overrides the search), so
 * single-GPU hosts need not have it.  One communicator per process. */
#define DR_COMM_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */
/* every rank, local: binds librccl and checks its version against the ABI subset this library declares -- DR_OK or the
 * reason, without talking to any other rank (so a host can agree on "every rank can" BEFORE anyone blocks in dr_comm_init) */
int dr_comm_available(void);
/* rank 0: ncclGetUniqueId into id_out[DR_COMM_ID_BYTES] */
int dr_comm_unique_id(void* id_out, uint64_t cap);
/* every rank, after dr_init: ncclCommInitRank(world, id, rank); blocks until all ranks have called it */
int dr_comm_init(int32_t rank, int32_t world, const void* unique_id, uint64_t id_bytes);
/* film_dev: [npixels][4] f32 (X, Y, Z, weightSum) on every rank; summed in place into rank `root`'s buffer on
 * the given hipStream_t (asynchronous like dr_render_device; other ranks' buffers are left as they were).
 * world == 1: no-op through the same code path (an in-place single-rank ncclReduce). */
int dr_film_reduce(void* film_dev, int64_t npixels, int32_t root, void* hip_stream);
/* in-place ncclAllReduce(max / sum) of n doubles on the stream: the barrier + max-over-ranks of a timed region */
int dr_comm_allreduce_f64(void* buf_dev, int64_t n, int32_t op_max, void* hip_stream);
/* One rank's part of a sharded render and the merge, in one call (the fan-out of RenderManager,
 * lib/dartray_web/render_manager.dart:100-141, with the rectangle copies replaced by ONE reduce): renders desc's share
 * (tile_rank / tile_count / tile_size, or task_num / task_count) into a zero-initialised full-frame device film,
 * sums the ranks' films on `root` through the communicator of dr_comm_init (skipped when none exists or its world
 * is 1), and on the root rank resolves the film and copies it out.  film_out / rgb_out ([h*w*4] / [h*w*3] f32) may be
 * NULL; on ranks other than root nothing is written.  A foreign host needs no device-memory calls of its own. */
int dr_render_sharded(DrScene* scene, const DrRenderDesc* desc, int32_t root, float* film_out, float* rgb_out);
int dr_comm_rank(void);  /* -1 before dr_comm_init */
int dr_comm_world(void); /* 0 before dr_comm_init */
int dr_comm_destroy(void);

const char* dr_last_error(void);
const char* dr_version(void);
/* The layout version of this header's structs and the meaning of its entry points.  A host compares dr_abi_version() of the library it
 * loaded with the DR_ABI_VERSION it was built against BEFORE it passes a struct: the structs carry no size field, so a host built against
 * an older header would hand the library a shorter object than it reads (version 5 -> 6: DrRenderDesc grew by tail_offsets, 1344 -> 1352
 * bytes; version 6 -> 7: DR_INTEGRATOR_DIRECT_ONE, dr_scene_workspace_bytes, the switch list of dr_set_option;
 * 8: DR_SAMPLER_STRATIFIED, strat_xsamples -- the former padding at offset 1292 -- and dr_generate_samples;
 * 9: DR_SAMPLER_ADAPTIVE -- minSamples travels in strat_xsamples, no layout change -- and dr_scene_get_adaptive_pixels.
 * Still 9: DR_SAMPLER_HALTON and dr_generate_halton_samples are additive -- a new constant and a new entry point, no struct changes, no
 * existing call means anything else; a host built against the earlier version-9 header runs unchanged.  Likewise dr_loop_subdivide and
 * dr_loop_subdivide_device: two new entry points, no struct; and DR_SAMPLER_RANDOM: a new constant that dr_render*, dr_generate_samples and
 * dr_scene_last_render_info serve like the other pixel-bound modes, no struct, no entry point; and DR_INTEGRATOR_WHITTED: a new constant for
 * DrRenderDesc.integrator, whose max_depth carries maxdepth -- no struct, no field, no entry point; dr_scene_last_render_info names it in the
 * word that was reserved, which stays -1 after every other integrator's render; and DR_INTEGRATOR_AO: a new constant whose three parameters
 * travel in storage no render read under the constants a version-9 host can pass -- ao_nsamples in the padding behind sample_stride, ao_mindist /
 * ao_maxdist in unions with tail / tail_offsets, which that integrator does not read -- so no field moved, the struct keeps its 1352 bytes, and a
 * host built against the earlier version-9 header, which never names the constant, runs unchanged; and DR_INTEGRATOR_FEATURE: a new constant
 * whose channel travels in the padding behind max_tail, read under that constant only, and one new entry point, dr_feature_check; and the
 * denoiser: one new struct, DrDenoiseParams, that only its three new entry points read -- dr_denoise_atrous_host, dr_denoise_atrous and
 * dr_denoise_atrous_device -- no existing struct, constant or call means anything else; and DR_INTEGRATOR_DIFFUSE_PRT: a new constant whose two
 * parameters are union members at the offsets of ao_nsamples (prt_nsamples) and feature_channel (prt_lmax) -- storage that is read under one
 * integrator's constant only -- and two new entry points, dr_prt_incident and dr_sh_evaluate: no field moved, 1352 bytes; and
 * DR_INTEGRATOR_GLOSSY_PRT: a new constant that reads the same two union members, one new struct, DrGlossyPrtParams, that only its new entry point
 * dr_scene_set_glossy_prt reads, and four more new entry points: dr_prt_bsdf_matrix, dr_sh_rotate, dr_sh_bsdf_matrix_host, dr_sh_rotate_device; and
 * DR_INTEGRATOR_USE_PROBES: a new constant that reads no field of DrRenderDesc beyond the common ones, one new struct, DrProbesDesc, that only
 * the new entry points read -- dr_probes_surface_points, dr_probes_grid, dr_probes_candidates, dr_probes_bake -- and dr_scene_set_probes: nothing
 * existing moved or changed its meaning, so the version stays 9; and the pair denoiser: one new struct, DrDenoisePairParams, that only its
 * three new entry points read -- dr_denoise_pair_host, dr_denoise_pair and dr_denoise_pair_device; and the display transform: one new struct,
 * DrDisplayParams, that only its seven new entry points read -- dr_display_check, dr_display_table, dr_display_host, dr_display,
 * dr_display_device, dr_display_exposure_host and dr_display_exposure; and the NURBS shape: one new struct, DrNurbsPatch, that only its
 * two new entry points read -- dr_nurbs_dice and dr_nurbs_dice_device; and the upsampler: one new struct, DrUpsampleParams, that only its
 * four new entry points read -- dr_upsample_check, dr_upsample_host, dr_upsample and dr_upsample_device; and temporal accumulation: one new
 * struct, DrTemporalParams, that only its four new entry points read -- dr_temporal_check, dr_temporal_host, dr_temporal and
 * dr_temporal_device; and the moments denoiser: one new struct, DrDenoiseMomentsParams, that only its four new entry points read --
 * dr_denoise_moments_check, dr_denoise_moments_host, dr_denoise_moments and dr_denoise_moments_device; and firefly suppression: one new
 * struct, DrFireflyParams, that only its four new entry points read -- dr_firefly_check, dr_firefly_host, dr_firefly and
 * dr_firefly_device; and the one-pass guide render: one new struct, DrGuidesDesc, that only its three new entry points read --
 * dr_render_guides_check, dr_render_guides and dr_render_guides_device; no field of DrRenderDesc moved; and DR_INTEGRATOR_MATERIAL: a new
 * constant whose channel is a third member of feature_channel's union, read under that constant only, and one new entry point,
 * dr_material_check; and demodulation: one new struct, DrDemodulateParams, that only its seven new entry points read -- dr_demodulate_check,
 * dr_demodulate_host, dr_demodulate, dr_demodulate_device, dr_remodulate_host, dr_remodulate and dr_remodulate_device; and dr_scene_get_table_counts:
 * one new read-only entry point, no struct). */
#define DR_ABI_VERSION 9
int32_t dr_abi_version(void);

/* Tuning / diagnostic switches.  Every switch is also an environment variable of the same name (DARTRAY_<NAME>); a
 * value set here takes precedence, is read at every use (nothing is latched at first use: the next render sees it) and
 * needs no setenv in a long-lived foreign host.  name: with or without the DARTRAY_ prefix, any case; value NULL: back
 * to the environment's value; "": unset for this process.  Unknown names are DR_ERR_INVALID.  The film never depends on a
 * switch, with one stated exception: the switches pick between bit-exact variants of a kernel, a layout or a schedule, or
 * print diagnostics.  The exception is the sampler: LAZY_GEN and the GEN_* switches choose when and how the device LD
 * sampler draws the same keyed streams -- bit-exact by test (tests/test_gpu_render.py, test_gpu_options.py), but they are
 * variants of the sampler, not of a schedule.  The fifteen switches (round 6; the A/B switches of measured negatives left the library with their
 * code: experiments/r06_*.diff):
 *   TRACE_IMPL 2|3|5      traversal kernels for both ray kinds: 2 = k_trace<0/1>, 3 = the sibling-pair kernels k_trace3<0> / k_trace3a,
 *                         5 = 3 with the closest-hit rays' cold state in LDS (k_trace3c); default: the scene's measured choice
 *   TRACE_WG_PER_CU n     workgroups of a persistent traversal launch per CU (occupancy sweeps)
 *   STATE_LAYOUT 64|4     path-state layout (default: picked per scene from the pilot's stage-list densities)
 *   BATCH_BITS b          at most 2^b camera samples per batch (16..28; default 27 for a scene's first big render, 28 afterwards)
 *   OVERLAP_ANY 0         a stage's any-hit launch after its closest-hit launch instead of beside it
 *   PILOT 0|force         no calibration batches / calibration batches also on renders too small to need them (tests)
 *   COHERENT_CAMERA 0     the camera rays through the per-lane traversal kernels like every other ray (default: the wave-coherent k_trace_pk)
 *   LAZY_GEN 0            the device sampler shuffles every LD block for every pixel up front (default: bounce b's blocks only for the
 *                         64-pixel groups that still have a path alive at bounce b)
 *   GEN_ALL_BLOCKS 1      ... and also the blocks no kernel reads;  GEN_SLOW_DRAWS 1   every generator step through Random.nextInt's retry loop
 *   SCENE_PREP host       dr_scene_create's tree checks and pair records by the serial host loops (the reference the device code is tested against)
 *   BUILD_THREADS n       threads of the host BVH builder;  RCCL_LIB path   the librccl to bind
 *   STAGE_COUNTS 1|2      per stage: list lengths and kernel times (2: also the node visits / triangle tests of each stage's traversals,
 *                         waiting for the device after every stage);  VERBOSE 1|2   what the library decided (2: + the BVH builders' timings) */
int dr_set_option(const char* name, const char* value);


/* ---- layout checks: a foreign host (dart:ffi Struct classes, ctypes, a C program) must see exactly these
 * sizes and offsets (LP64, little endian, natural alignment) ---- */
#ifdef __cplusplus
#define DR_ABI_ASSERT(c, m) static_assert(c, m)
#else
#define DR_ABI_ASSERT(c, m) _Static_assert(c, m)
#endif
#define DR_ABI_SIZE(T, n) DR_ABI_ASSERT(sizeof(T) == (n), "sizeof(" #T ") != " #n)
#define DR_ABI_OFFSET(T, f, n) DR_ABI_ASSERT(offsetof(T, f) == (n), "offsetof(" #T ", " #f ") != " #n)
DR_ABI_SIZE(DrBvhNode, 32);
DR_ABI_OFFSET(DrBvhNode, offset, 24);
DR_ABI_OFFSET(DrBvhNode, nprims, 28);
DR_ABI_OFFSET(DrBvhNode, axis, 30);
DR_ABI_SIZE(DrMaterial, 56);
DR_ABI_OFFSET(DrMaterial, kd, 4);
DR_ABI_OFFSET(DrMaterial, sigma, 40);
DR_ABI_OFFSET(DrMaterial, index, 48);
DR_ABI_SIZE(DrAreaLight, 128);
DR_ABI_OFFSET(DrAreaLight, first_tri, 16);
DR_ABI_OFFSET(DrAreaLight, position, 32);
DR_ABI_OFFSET(DrAreaLight, world_to_light, 48);
DR_ABI_OFFSET(DrAreaLight, cone_width, 112);
DR_ABI_SIZE(DrEnvMap, 144);
DR_ABI_OFFSET(DrEnvMap, width, 8);
DR_ABI_OFFSET(DrEnvMap, light_to_world, 16);
DR_ABI_SIZE(DrLightTri, 16);
DR_ABI_SIZE(DrMeshXform, 128);
DR_ABI_SIZE(DrQuadric, 168);
DR_ABI_OFFSET(DrQuadric, object_to_world, 8);
DR_ABI_OFFSET(DrQuadric, params, 136);
DR_ABI_SIZE(DrSceneDesc, 208);
DR_ABI_OFFSET(DrSceneDesc, nnodes, 8);
DR_ABI_OFFSET(DrSceneDesc, verts, 16);
DR_ABI_OFFSET(DrSceneDesc, tri_idx, 32);
DR_ABI_OFFSET(DrSceneDesc, tri_material, 48);
DR_ABI_OFFSET(DrSceneDesc, materials, 72);
DR_ABI_OFFSET(DrSceneDesc, nmaterials, 80);
DR_ABI_OFFSET(DrSceneDesc, lights, 88);
DR_ABI_OFFSET(DrSceneDesc, nlights, 96);
DR_ABI_OFFSET(DrSceneDesc, light_tris, 104);
DR_ABI_OFFSET(DrSceneDesc, nlight_tris, 112);
DR_ABI_OFFSET(DrSceneDesc, bvh_depth, 116);
DR_ABI_OFFSET(DrSceneDesc, env_maps, 120);
DR_ABI_OFFSET(DrSceneDesc, quadrics, 136);
DR_ABI_OFFSET(DrSceneDesc, vert_normals, 152);
DR_ABI_OFFSET(DrSceneDesc, mesh_xforms, 192);
DR_ABI_OFFSET(DrSceneDesc, nmesh_xforms, 200);
DR_ABI_SIZE(DrRay, 40);
DR_ABI_OFFSET(DrRay, tmin, 24);
DR_ABI_SIZE(DrHit, 32);
DR_ABI_OFFSET(DrHit, t, 8);
DR_ABI_SIZE(DrCamera, 168);
DR_ABI_OFFSET(DrCamera, lens_radius, 128);
DR_ABI_OFFSET(DrCamera, focal_distance, 136);
DR_ABI_OFFSET(DrCamera, type, 160);
DR_ABI_SIZE(DrFilm, 1080);
DR_ABI_OFFSET(DrFilm, crop, 8);
DR_ABI_OFFSET(DrFilm, filter_xw, 40);
DR_ABI_OFFSET(DrFilm, filter_table, 56);
DR_ABI_SIZE(DrRenderDesc, 1352);
DR_ABI_OFFSET(DrRenderDesc, film, 168);
DR_ABI_OFFSET(DrRenderDesc, integrator, 1248);
DR_ABI_OFFSET(DrRenderDesc, seed, 1264);
DR_ABI_OFFSET(DrRenderDesc, task_num, 1272);
DR_ABI_OFFSET(DrRenderDesc, tile_rank, 1280);
DR_ABI_OFFSET(DrRenderDesc, strat_xsamples, 1292);
DR_ABI_OFFSET(DrRenderDesc, nsamples, 1296);
DR_ABI_OFFSET(DrRenderDesc, pixel_xy, 1304);
DR_ABI_OFFSET(DrRenderDesc, sample_vec, 1312);
DR_ABI_OFFSET(DrRenderDesc, sample_stride, 1320);
DR_ABI_OFFSET(DrRenderDesc, ao_nsamples, 1324);
DR_ABI_OFFSET(DrRenderDesc, tail, 1328);
DR_ABI_OFFSET(DrRenderDesc, ao_mindist, 1328);
DR_ABI_OFFSET(DrRenderDesc, max_tail, 1336);
DR_ABI_OFFSET(DrRenderDesc, feature_channel, 1340);
DR_ABI_OFFSET(DrRenderDesc, material_channel, 1340);
DR_ABI_OFFSET(DrRenderDesc, prt_nsamples, 1324);
DR_ABI_OFFSET(DrRenderDesc, prt_lmax, 1340);
DR_ABI_OFFSET(DrRenderDesc, tail_offsets, 1344);
DR_ABI_OFFSET(DrRenderDesc, ao_maxdist, 1344);
DR_ABI_SIZE(DrRenderStats, 200);
DR_ABI_OFFSET(DrRenderStats, trace_ms, 72);
DR_ABI_OFFSET(DrRenderStats, film_ms, 144);
DR_ABI_OFFSET(DrRenderStats, shade_items, 152);
DR_ABI_OFFSET(DrRenderStats, pilot_ms, 192);
DR_ABI_SIZE(DrDenoiseParams, 16);
DR_ABI_OFFSET(DrDenoiseParams, k_color, 4);
DR_ABI_OFFSET(DrDenoiseParams, k_normal, 8);
DR_ABI_OFFSET(DrDenoiseParams, k_depth, 12);
DR_ABI_SIZE(DrDenoisePairParams, 20);
DR_ABI_OFFSET(DrDenoisePairParams, k_color, 4);
DR_ABI_OFFSET(DrDenoisePairParams, k_depth, 12);
DR_ABI_OFFSET(DrDenoisePairParams, var_floor, 16);
DR_ABI_SIZE(DrDisplayParams, 32);
DR_ABI_OFFSET(DrDisplayParams, permille, 12);
DR_ABI_OFFSET(DrDisplayParams, exposure, 16);
DR_ABI_OFFSET(DrDisplayParams, invalid_rgba, 28);
DR_ABI_SIZE(DrNurbsPatch, 72);
DR_ABI_OFFSET(DrNurbsPatch, uknots, 8);
DR_ABI_OFFSET(DrNurbsPatch, nv, 24);
DR_ABI_OFFSET(DrNurbsPatch, cp, 48);
DR_ABI_OFFSET(DrNurbsPatch, dicev, 64);
DR_ABI_SIZE(DrUpsampleParams, 16);
DR_ABI_OFFSET(DrUpsampleParams, taps, 4);
DR_ABI_OFFSET(DrUpsampleParams, k_normal, 8);
DR_ABI_OFFSET(DrUpsampleParams, k_depth, 12);
DR_ABI_SIZE(DrTemporalParams, 400);
DR_ABI_OFFSET(DrTemporalParams, cur_to_prev, 128);
DR_ABI_OFFSET(DrTemporalParams, prev_to_raster, 256);
DR_ABI_OFFSET(DrTemporalParams, depth_tol, 384);
DR_ABI_OFFSET(DrTemporalParams, normal_tol, 388);
DR_ABI_OFFSET(DrTemporalParams, max_history, 392);
DR_ABI_SIZE(DrDenoiseMomentsParams, 28);
DR_ABI_OFFSET(DrDenoiseMomentsParams, k_color, 4);
DR_ABI_OFFSET(DrDenoiseMomentsParams, var_floor, 16);
DR_ABI_OFFSET(DrDenoiseMomentsParams, min_history, 20);
DR_ABI_OFFSET(DrDenoiseMomentsParams, radius, 24);
DR_ABI_SIZE(DrDemodulateParams, 4);
DR_ABI_SIZE(DrFireflyParams, 24);
DR_ABI_OFFSET(DrFireflyParams, rank, 4);
DR_ABI_OFFSET(DrFireflyParams, threshold, 8);
DR_ABI_OFFSET(DrFireflyParams, floor, 12);
DR_ABI_OFFSET(DrFireflyParams, depth_tol, 16);
DR_ABI_OFFSET(DrFireflyParams, normal_tol, 20);
DR_ABI_SIZE(DrGuidesDesc, 24);
DR_ABI_OFFSET(DrGuidesDesc, channels, 4);

#ifdef __cplusplus
}
#endif
#endif /* DARTRAY_HIP_H */
