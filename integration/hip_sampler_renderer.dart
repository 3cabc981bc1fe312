/****************************************************************************
 * hip_sampler_renderer.dart -- DartRay's Renderer seam on an MI355X.
 *
 * Drop this file into lib/renderers/ of brendan-duncan/dartray and add the
 * `hipsampler` branch of INTEGRATION.md section 2 to DartRay._makeRenderer
 * (lib/dartray/dartray.dart:662-761).  `HipSamplerRenderer.render(Scene)`
 * (Renderer.render, lib/core/renderer.dart:27-35) flattens the Scene the
 * Dart API built -- BVHAccel.nodes / .primitives (bvh_accel.dart:486-487,
 * :533-538), every GeometricPrimitive's shape / material / areaLight
 * (geometric_primitive.dart:83-85), the world-space vertices of its
 * TriangleMesh (triangle_mesh.dart:39-42), each DiffuseAreaLight's ShapeSet
 * in ShapeSet order (shape_set.dart:27-35), scene.lights in list order --
 * into the POD structs of include/dartray_hip.h and renders it with
 * libdartray_hip.so through dart:ffi.  The OutputImage it returns
 * (output_image.dart:35-55) is what SamplerRenderer.render returns.
 *
 * Structs are written field by field into native memory at the byte offsets
 * the header itself asserts (DR_ABI_SIZE / DR_ABI_OFFSET at the end of
 * dartray_hip.h); tests/test_abi_c_host.py checks every offset constant of
 * this file against those asserts.  No Dart SDK exists in the image this was
 * written in: the file has been checked against the header mechanically,
 * not executed.  tests/abi/c1_from_c.c is the same call sequence from C and
 * IS executed on the GPU.
 *
 * SDK window: the reference is pre-null-safety Dart (no `environment` in its pubspec.yaml) and dart:ffi with
 * package:ffi's `calloc` / `Utf8.toDartString` needs Dart >= 2.12: Dart 2.12 ... 2.19 with `// @dart=2.9`-style
 * unsound null safety (`dart --no-sound-null-safety`), package:ffi ^1.0.0.  Dart 3 rejects the reference itself.
 *
 * Scope: what the device path covers (SURVEY.md section 8): BVHAccel over
 * TriangleMesh / Sphere / Disk shapes, matte / mirror / glass / plastic
 * materials with constant textures, DiffuseAreaLight / InfiniteAreaLight /
 * point, spot and distant lights, PathIntegrator and DirectLightingIntegrator
 * ("all"), the low-discrepancy, the stratified and the adaptive sampler, ImageFilm with any Filter, the three
 * cameras.  Anything else is reported through LogSevere (log.dart:42-47),
 * never approximated.
 ****************************************************************************/
library hip_sampler_renderer;

import 'dart:async';
import 'dart:ffi';
import 'dart:typed_data';

import 'package:ffi/ffi.dart';

import '../accelerators/accelerators.dart';
import '../cameras/cameras.dart';
import '../core/core.dart';
import '../film/film.dart';
import '../lights/lights.dart';
import '../materials/materials.dart';
import '../samplers/samplers.dart';
import '../shapes/shapes.dart';
import '../surface_integrators/surface_integrators.dart';

// ---- sizes and byte offsets of include/dartray_hip.h (DR_ABI_SIZE / DR_ABI_OFFSET) ----
const int SIZEOF_DrBvhNode = 32;
const int OFF_DrBvhNode_bmin = 0;
const int OFF_DrBvhNode_bmax = 12;
const int OFF_DrBvhNode_offset = 24;
const int OFF_DrBvhNode_nprims = 28;
const int OFF_DrBvhNode_axis = 30;
const int SIZEOF_DrMaterial = 56;
const int OFF_DrMaterial_type = 0;
const int OFF_DrMaterial_kd = 4;
const int OFF_DrMaterial_kr = 16;
const int OFF_DrMaterial_kt = 28;
const int OFF_DrMaterial_sigma = 40;
const int OFF_DrMaterial_index = 48;
const int SIZEOF_DrAreaLight = 128;
const int OFF_DrAreaLight_L = 0;
const int OFF_DrAreaLight_nsamples = 12;
const int OFF_DrAreaLight_first_tri = 16;
const int OFF_DrAreaLight_ntris = 20;
const int OFF_DrAreaLight_kind = 24;
const int OFF_DrAreaLight_env_index = 28;
const int OFF_DrAreaLight_position = 32;
const int OFF_DrAreaLight_world_to_light = 48;
const int OFF_DrAreaLight_cone_width = 112;
const int OFF_DrAreaLight_cone_falloff_start = 120;
const int SIZEOF_DrEnvMap = 144;
const int OFF_DrEnvMap_texels = 0;
const int OFF_DrEnvMap_width = 8;
const int OFF_DrEnvMap_height = 12;
const int OFF_DrEnvMap_light_to_world = 16;
const int OFF_DrEnvMap_world_to_light = 80;
const int SIZEOF_DrLightTri = 16;
const int OFF_DrLightTri_v = 0;
const int OFF_DrLightTri_reverse_orientation = 12;
const int SIZEOF_DrMeshXform = 128;
const int OFF_DrMeshXform_object_to_world = 0;
const int OFF_DrMeshXform_world_to_object = 64;
const int SIZEOF_DrQuadric = 168;
const int OFF_DrQuadric_kind = 0;
const int OFF_DrQuadric_object_to_world = 8;
const int OFF_DrQuadric_world_to_object = 72;
const int OFF_DrQuadric_params = 136;
const int SIZEOF_DrSceneDesc = 208;
const int OFF_DrSceneDesc_nodes = 0;
const int OFF_DrSceneDesc_nnodes = 8;
const int OFF_DrSceneDesc_verts = 16;
const int OFF_DrSceneDesc_nverts = 24;
const int OFF_DrSceneDesc_tri_idx = 32;
const int OFF_DrSceneDesc_ntris = 40;
const int OFF_DrSceneDesc_tri_material = 48;
const int OFF_DrSceneDesc_tri_light = 56;
const int OFF_DrSceneDesc_tri_reverse = 64;
const int OFF_DrSceneDesc_materials = 72;
const int OFF_DrSceneDesc_nmaterials = 80;
const int OFF_DrSceneDesc_lights = 88;
const int OFF_DrSceneDesc_nlights = 96;
const int OFF_DrSceneDesc_light_tris = 104;
const int OFF_DrSceneDesc_nlight_tris = 112;
const int OFF_DrSceneDesc_bvh_depth = 116;
const int OFF_DrSceneDesc_env_maps = 120;
const int OFF_DrSceneDesc_nenv_maps = 128;
const int OFF_DrSceneDesc_quadrics = 136;
const int OFF_DrSceneDesc_nquadrics = 144;
const int OFF_DrSceneDesc_vert_normals = 152;
const int OFF_DrSceneDesc_vert_tangents = 160;
const int OFF_DrSceneDesc_vert_uvs = 168;
const int OFF_DrSceneDesc_tri_shading = 176;
const int OFF_DrSceneDesc_tri_xform = 184;
const int OFF_DrSceneDesc_mesh_xforms = 192;
const int OFF_DrSceneDesc_nmesh_xforms = 200;
const int SIZEOF_DrCamera = 168;
const int OFF_DrCamera_raster_to_camera = 0;
const int OFF_DrCamera_camera_to_world = 64;
const int OFF_DrCamera_lens_radius = 128;
const int OFF_DrCamera_focal_distance = 136;
const int OFF_DrCamera_shutter_open = 144;
const int OFF_DrCamera_shutter_close = 152;
const int OFF_DrCamera_type = 160;
const int SIZEOF_DrFilm = 1080;
const int OFF_DrFilm_xres = 0;
const int OFF_DrFilm_yres = 4;
const int OFF_DrFilm_crop = 8;
const int OFF_DrFilm_filter_xw = 40;
const int OFF_DrFilm_filter_yw = 48;
const int OFF_DrFilm_filter_table = 56;
const int SIZEOF_DrRenderDesc = 1352;
const int OFF_DrRenderDesc_camera = 0;
const int OFF_DrRenderDesc_film = 168;
const int OFF_DrRenderDesc_integrator = 1248;
const int OFF_DrRenderDesc_max_depth = 1252;
const int OFF_DrRenderDesc_spp = 1256;
const int OFF_DrRenderDesc_sampler_mode = 1260;
const int OFF_DrRenderDesc_seed = 1264;
const int OFF_DrRenderDesc_task_num = 1272;
const int OFF_DrRenderDesc_task_count = 1276;
const int OFF_DrRenderDesc_tile_rank = 1280;
const int OFF_DrRenderDesc_tile_count = 1284;
const int OFF_DrRenderDesc_tile_size = 1288;
const int OFF_DrRenderDesc_strat_xsamples = 1292;  // DR_SAMPLER_STRATIFIED(_NOJITTER): xPixelSamples; DR_SAMPLER_ADAPTIVE: minSamples
const int OFF_DrRenderDesc_nsamples = 1296;
const int OFF_DrRenderDesc_pixel_xy = 1304;
const int OFF_DrRenderDesc_sample_vec = 1312;
const int OFF_DrRenderDesc_sample_stride = 1320;
const int OFF_DrRenderDesc_ao_nsamples = 1324;  // DR_INTEGRATOR_AO only (the former padding)
const int OFF_DrRenderDesc_tail = 1328;
const int OFF_DrRenderDesc_ao_mindist = 1328;  // DR_INTEGRATOR_AO only: a double in the tail pointer's storage (that integrator reads no tail)
const int OFF_DrRenderDesc_max_tail = 1336;
const int OFF_DrRenderDesc_feature_channel = 1340;  // DR_INTEGRATOR_FEATURE only (the former padding)
const int OFF_DrRenderDesc_material_channel = 1340;  // DR_INTEGRATOR_MATERIAL only (a member of the same union)
const int OFF_DrRenderDesc_prt_nsamples = 1324;  // DR_INTEGRATOR_DIFFUSE_PRT only: a union member at ao_nsamples' offset
const int OFF_DrRenderDesc_prt_lmax = 1340;  // DR_INTEGRATOR_DIFFUSE_PRT only: a union member at feature_channel's offset
const int OFF_DrRenderDesc_ao_maxdist = 1344;  // likewise, in the storage of tail_offsets
const int OFF_DrRenderDesc_tail_offsets = 1344;  // host-buffer sampler only: stays NULL here (calloc'd descriptor)
// DrDenoiseParams (the a-trous denoiser, DESIGN.md 2.15): int32 iterations (1 .. 8) at 0, then three f32 sharpness values k = 1 / sigma^2
const int SIZEOF_DrDenoiseParams = 16;
const int OFF_DrDenoiseParams_iterations = 0;
const int OFF_DrDenoiseParams_k_color = 4;
const int OFF_DrDenoiseParams_k_normal = 8;
const int OFF_DrDenoiseParams_k_depth = 12;
// DrDenoisePairParams (the variance-guided a-trous denoiser over two half renders, DESIGN.md 2.19): int32 iterations (1 .. 8) at 0, the three
// f32 sharpness values -- k_color in units of the local variance -- and the f32 variance floor (> 0)
const int SIZEOF_DrDenoisePairParams = 20;
const int OFF_DrDenoisePairParams_iterations = 0;
const int OFF_DrDenoisePairParams_k_color = 4;
const int OFF_DrDenoisePairParams_k_normal = 8;
const int OFF_DrDenoisePairParams_k_depth = 12;
const int OFF_DrDenoisePairParams_var_floor = 16;
// DrDisplayParams (the display transform, DESIGN.md 2.20): four uint32 -- the tone curve, the encode, auto-exposure on / off, the rank in
// permille --, three f32 -- the manual scale, the key, 1 / white^2 -- and the uint32 r | g << 8 | b << 16 | a << 24 of an invalid pixel
const int SIZEOF_DrDisplayParams = 32;
const int OFF_DrDisplayParams_curve = 0;
const int OFF_DrDisplayParams_encode = 4;
const int OFF_DrDisplayParams_auto_exposure = 8;
const int OFF_DrDisplayParams_permille = 12;
const int OFF_DrDisplayParams_exposure = 16;
const int OFF_DrDisplayParams_key = 20;
const int OFF_DrDisplayParams_inv_white2 = 24;
const int OFF_DrDisplayParams_invalid_rgba = 28;
// DrUpsampleParams (the joint bilateral upsampler, DESIGN.md 2.22): int32 factor (2 or 4) at 0, int32 taps (2 or 4) at 4, then the two f32
// sharpness values k = 1 / sigma^2 of the normal and the depth term
const int SIZEOF_DrUpsampleParams = 16;
const int OFF_DrUpsampleParams_factor = 0;
const int OFF_DrUpsampleParams_taps = 4;
const int OFF_DrUpsampleParams_k_normal = 8;
const int OFF_DrUpsampleParams_k_depth = 12;
// DrTemporalParams (temporal accumulation with reprojection, DESIGN.md 2.23): three row-major f64 4 x 4 matrices -- the current camera's
// raster-to-camera, current camera space to previous camera space, previous camera space to previous raster --, then f32 depth_tol (relative),
// f32 normal_tol (squared distance of the encoded normals), int32 max_history (1..4096) and a reserved uint32 that is 0
const int SIZEOF_DrTemporalParams = 400;
const int OFF_DrTemporalParams_raster_to_camera = 0;
const int OFF_DrTemporalParams_cur_to_prev = 128;
const int OFF_DrTemporalParams_prev_to_raster = 256;
const int OFF_DrTemporalParams_depth_tol = 384;
const int OFF_DrTemporalParams_normal_tol = 388;
const int OFF_DrTemporalParams_max_history = 392;
// DrDenoiseMomentsParams (the variance-guided a-trous denoiser over a temporal history, DESIGN.md 2.24): DrDenoisePairParams' five fields, then
// int32 min_history (2..4096: a history at least this long gives the temporal variance estimate) and int32 radius (0..3: the spatial one's window)
const int SIZEOF_DrDenoiseMomentsParams = 28;
const int OFF_DrDenoiseMomentsParams_iterations = 0;
const int OFF_DrDenoiseMomentsParams_k_color = 4;
const int OFF_DrDenoiseMomentsParams_k_normal = 8;
const int OFF_DrDenoiseMomentsParams_k_depth = 12;
const int OFF_DrDenoiseMomentsParams_var_floor = 16;
const int OFF_DrDenoiseMomentsParams_min_history = 20;
const int OFF_DrDenoiseMomentsParams_radius = 24;
// DrFireflyParams (firefly suppression, the outlier clamp ahead of the filters, DESIGN.md 2.25): int32 radius (1 or 2: the window is
// (2 radius + 1)^2 pixels), int32 rank (1..4: the member luminance the limit is taken from), f32 threshold and f32 floor (the limit is
// threshold * m + floor), then DrTemporalParams' f32 depth_tol and f32 normal_tol
const int SIZEOF_DrFireflyParams = 24;
const int OFF_DrFireflyParams_radius = 0;
const int OFF_DrFireflyParams_rank = 4;
const int OFF_DrFireflyParams_threshold = 8;
const int OFF_DrFireflyParams_floor = 12;
const int OFF_DrFireflyParams_depth_tol = 16;
const int OFF_DrFireflyParams_normal_tol = 20;
// DrNurbsPatch (one NURBS patch, DESIGN.md 2.21): per direction int32 n, int32 order, the address of n + order f32 knots and the f32 range;
// the address of the nu * nv control points (3 floats each, or 4 when homogeneous is 1); uint32 dice rates (0: 30)
const int SIZEOF_DrNurbsPatch = 72;
const int OFF_DrNurbsPatch_nu = 0;
const int OFF_DrNurbsPatch_uorder = 4;
const int OFF_DrNurbsPatch_uknots = 8;
const int OFF_DrNurbsPatch_u0 = 16;
const int OFF_DrNurbsPatch_u1 = 20;
const int OFF_DrNurbsPatch_nv = 24;
const int OFF_DrNurbsPatch_vorder = 28;
const int OFF_DrNurbsPatch_vknots = 32;
const int OFF_DrNurbsPatch_v0 = 40;
const int OFF_DrNurbsPatch_v1 = 44;
const int OFF_DrNurbsPatch_cp = 48;
const int OFF_DrNurbsPatch_homogeneous = 56;
const int OFF_DrNurbsPatch_diceu = 60;
const int OFF_DrNurbsPatch_dicev = 64;
const int DR_NURBS_MAX_ORDER = 8;
const int DR_TONE_CLAMP = 0, DR_TONE_REINHARD = 1, DR_TONE_FILMIC = 2;
const int DR_ENCODE_SRGB = 0, DR_ENCODE_GAMMA22 = 1, DR_ENCODE_REFERENCE = 2;
const int DR_DISPLAY_BINS = 2048;

// enums of the header
const int DR_MATERIAL_MATTE = 0, DR_MATERIAL_MIRROR = 1, DR_MATERIAL_GLASS = 2, DR_MATERIAL_PLASTIC = 3;
const int DR_LIGHT_DIFFUSE_AREA = 0, DR_LIGHT_INFINITE = 1, DR_LIGHT_POINT = 2, DR_LIGHT_SPOT = 3, DR_LIGHT_DISTANT = 4;
const int DR_LIGHT_SPOT_COS = 5;
const int DR_SHADING_N = 1, DR_SHADING_S = 2, DR_SHADING_UV = 4;
const int DR_COMM_ID_BYTES = 128;
const int DR_PRIM_QUADRIC = 0xFFFFFFFF, DR_QUADRIC_SPHERE = 1, DR_QUADRIC_DISK = 2;
const int DR_CAMERA_PERSPECTIVE = 0, DR_CAMERA_ORTHOGRAPHIC = 1, DR_CAMERA_ENVIRONMENT = 2;
const int DR_INTEGRATOR_DIRECT_ALL = 0, DR_INTEGRATOR_PATH = 1, DR_INTEGRATOR_DIRECT_ONE = 2, DR_INTEGRATOR_WHITTED = 3, DR_INTEGRATOR_AO = 4;
const int DR_INTEGRATOR_FEATURE = 5;  // the first-hit feature integrator (FeatureIntegrator below): DrRenderDesc.feature_channel
const int DR_INTEGRATOR_DIFFUSE_PRT = 7;  // DiffusePRTIntegrator (6 is unassigned): DrRenderDesc.prt_nsamples / prt_lmax
const int DR_INTEGRATOR_GLOSSY_PRT = 9;  // GlossyPRTIntegrator (8 is unassigned): the same two fields; Kd, Ks, roughness by dr_scene_set_glossy_prt
// DrGlossyPrtParams: f32 Kd[3] at 0, f32 Ks[3] at 12, f64 roughness at 24
const int SIZEOF_DrGlossyPrtParams = 32, OFF_DrGlossyPrtParams_Kd = 0, OFF_DrGlossyPrtParams_Ks = 12, OFF_DrGlossyPrtParams_roughness = 24;
const int DR_INTEGRATOR_USE_PROBES = 11;  // UseProbesIntegrator (10 is unassigned): the grid by dr_scene_set_probes; no field of its own
// DrProbesDesc: i32 lmax at 0, include_indirect (must be 0) at 4, npoints at 8, has_bounds at 12, f32 bounds[6] at 16, f32 camera_pos[3] at 40,
// f64 spacing at 56, f64 time at 64
const int SIZEOF_DrProbesDesc = 72, OFF_DrProbesDesc_lmax = 0, OFF_DrProbesDesc_include_indirect = 4, OFF_DrProbesDesc_npoints = 8,
    OFF_DrProbesDesc_has_bounds = 12, OFF_DrProbesDesc_bounds = 16, OFF_DrProbesDesc_camera_pos = 40, OFF_DrProbesDesc_spacing = 56,
    OFF_DrProbesDesc_time = 64;
const int DR_INTEGRATOR_MATERIAL = 13;  // the first-hit material integrator (MaterialIntegrator below; 12 is unassigned): DrRenderDesc.material_channel
const int DR_MATERIAL_CHANNEL_ALBEDO = 0, DR_MATERIAL_CHANNEL_EMISSION = 1;
// DrDemodulateParams (demodulation around the image stages, DESIGN.md 2.27): f32 eps (finite, > 0; 1e-3 by default)
const int SIZEOF_DrDemodulateParams = 4;
const int OFF_DrDemodulateParams_eps = 0;
const int DR_FEATURE_NG = 0, DR_FEATURE_NS = 1, DR_FEATURE_DEPTH = 2, DR_FEATURE_UV = 3, DR_FEATURE_ID = 4;
// DrGuidesDesc (the channels of a guide render, DESIGN.md 2.26): int32 count (1..5), then int32 channels[5], DR_FEATURE_* values, none twice
const int DR_GUIDES_MAX = 5;
const int SIZEOF_DrGuidesDesc = 24;
const int OFF_DrGuidesDesc_count = 0;
const int OFF_DrGuidesDesc_channels = 4;
const int DR_SAMPLER_COUNTER = 1;
const int DR_SAMPLER_STRATIFIED = 2;           // StratifiedSampler on keyed streams; spp = xPixelSamples * yPixelSamples
const int DR_SAMPLER_STRATIFIED_NOJITTER = 3;  // ... with jitterSamples == false
const int DR_SAMPLER_ADAPTIVE = 4;             // AdaptiveSampler (contrast) on the LD sampler's keyed streams; spp = maxSamples
const int DR_SAMPLER_HALTON = 5;               // HaltonSampler: one sequence per task, samples not bound to pixels; spp = samplesPerPixel, any count
const int DR_SAMPLER_RANDOM = 6;               // RandomSampler: every value one nextDouble() of the (pixel, sample) stream; spp = samplesPerPixel, a power of two

typedef _InitC = Int32 Function(Int32);
typedef _InitD = int Function(int);
typedef _SceneCreateC = Int32 Function(Pointer<Uint8>, Pointer<Pointer<Void>>);
typedef _SceneCreateD = int Function(Pointer<Uint8>, Pointer<Pointer<Void>>);
typedef _RenderC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Pointer<Float>, Pointer<Float>);
typedef _RenderD = int Function(Pointer<Void>, Pointer<Uint8>, Pointer<Float>, Pointer<Float>);
typedef _RenderShardedC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Int32, Pointer<Float>, Pointer<Float>);
typedef _RenderShardedD = int Function(Pointer<Void>, Pointer<Uint8>, int, Pointer<Float>, Pointer<Float>);
typedef _RenderDeviceC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Pointer<Void>, Pointer<Void>);
typedef _RenderDeviceD = int Function(Pointer<Void>, Pointer<Uint8>, Pointer<Void>, Pointer<Void>);
typedef _FilmReduceC = Int32 Function(Pointer<Void>, Int64, Int32, Pointer<Void>);
typedef _FilmReduceD = int Function(Pointer<Void>, int, int, Pointer<Void>);
typedef _FilmResolveC = Int32 Function(Pointer<Void>, Int64, Pointer<Void>, Pointer<Void>);
typedef _FilmResolveD = int Function(Pointer<Void>, int, Pointer<Void>, Pointer<Void>);
typedef _CommIdC = Int32 Function(Pointer<Uint8>, Uint64);
typedef _CommIdD = int Function(Pointer<Uint8>, int);
typedef _CommInitC = Int32 Function(Int32, Int32, Pointer<Uint8>, Uint64);
typedef _CommInitD = int Function(int, int, Pointer<Uint8>, int);
typedef _CommVoidC = Int32 Function();
typedef _SetOptionC = Int32 Function(Pointer<Utf8>, Pointer<Utf8>);
typedef _SetOptionD = int Function(Pointer<Utf8>, Pointer<Utf8>);
typedef _SetGlossyPrtC = Int32 Function(Pointer<Void>, Pointer<Uint8>);  // (scene, DrGlossyPrtParams*)
typedef _SetGlossyPrtD = int Function(Pointer<Void>, Pointer<Uint8>);
// radiance probes (DESIGN.md 2.18): (scene, data, n); (scene, DrProbesDesc*, out, nfloats); (scene, DrProbesDesc*, nprobes[3], bounds[6]);
// (scene, camera_pos[3], time, npoints, out, count*); (scene, DrProbesDesc*, points, npoints, nfound*, accepted*)
typedef _SetProbesC = Int32 Function(Pointer<Void>, Pointer<Float>, Int64);
typedef _SetProbesD = int Function(Pointer<Void>, Pointer<Float>, int);
typedef _ProbesBakeC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Pointer<Float>, Int64);
typedef _ProbesBakeD = int Function(Pointer<Void>, Pointer<Uint8>, Pointer<Float>, int);
typedef _ProbesGridC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Pointer<Int32>, Pointer<Float>);
typedef _ProbesGridD = int Function(Pointer<Void>, Pointer<Uint8>, Pointer<Int32>, Pointer<Float>);
typedef _ProbesPointsC = Int32 Function(Pointer<Void>, Pointer<Float>, Double, Int32, Pointer<Float>, Pointer<Int32>);
typedef _ProbesPointsD = int Function(Pointer<Void>, Pointer<Float>, double, int, Pointer<Float>, Pointer<Int32>);
typedef _ProbesCandidatesC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Pointer<Float>, Int32, Pointer<Int32>, Pointer<Int32>);
typedef _ProbesCandidatesD = int Function(Pointer<Void>, Pointer<Uint8>, Pointer<Float>, int, Pointer<Int32>, Pointer<Int32>);
typedef _SetLayoutC = Int32 Function(Pointer<Void>, Int32);
typedef _SetLayoutD = int Function(Pointer<Void>, int);
typedef _CommVoidD = int Function();
typedef _KernelsC = Int32 Function(Pointer<Void>, Pointer<Uint32>);
typedef _KernelsD = int Function(Pointer<Void>, Pointer<Uint32>);
typedef _GetLayoutC = Int32 Function(Pointer<Void>, Pointer<Int32>, Pointer<Float>);
typedef _GetLayoutD = int Function(Pointer<Void>, Pointer<Int32>, Pointer<Float>);
typedef _AdaptivePixelsC = Int32 Function(Pointer<Void>, Pointer<Int32>, Uint64, Pointer<Uint64>);
typedef _AdaptivePixelsD = int Function(Pointer<Void>, Pointer<Int32>, int, Pointer<Uint64>);
typedef _HaltonSamplesC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Uint64, Uint64, Pointer<Uint64>, Pointer<Int32>, Pointer<Float>, Int32,
    Pointer<Uint64>);
typedef _HaltonSamplesD = int Function(Pointer<Void>, Pointer<Uint8>, int, int, Pointer<Uint64>, Pointer<Int32>, Pointer<Float>, int,
    Pointer<Uint64>);
// dr_loop_subdivide / dr_loop_subdivide_device (LoopSubdivision.refine on the host / on the GPU; DESIGN.md 2.10): indices, nfaces, P, nverts,
// nlevels, P_out, N_out, indices_out, vert_cap, face_cap, nverts_out, nfaces_out.  All three outputs null: the size query.  (Signatures only --
// like the rest of this file they have never been compiled: nothing here can compile Dart.)
typedef _LoopSubdivideC = Int32 Function(Pointer<Uint32>, Uint64, Pointer<Float>, Uint64, Int32, Pointer<Float>, Pointer<Float>, Pointer<Uint32>,
    Uint64, Uint64, Pointer<Uint64>, Pointer<Uint64>);
typedef _LoopSubdivideD = int Function(Pointer<Uint32>, int, Pointer<Float>, int, int, Pointer<Float>, Pointer<Float>, Pointer<Uint32>,
    int, int, Pointer<Uint64>, Pointer<Uint64>);
// dr_nurbs_dice / dr_nurbs_dice_device (Nurbs.refine on the host / on the GPU; DESIGN.md 2.21): DrNurbsPatch (72 bytes, the OFF_DrNurbsPatch_*
// offsets above), P_out, N_out, uv_out, indices_out, vert_capacity, tri_capacity, nverts, ntris.  All four outputs null: the size query.
// (Signatures only, never compiled, like the rest.)
typedef _NurbsDiceC = Int32 Function(Pointer<Uint8>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Uint32>, Uint64, Uint64,
    Pointer<Uint64>, Pointer<Uint64>);
typedef _NurbsDiceD = int Function(Pointer<Uint8>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Uint32>, int, int,
    Pointer<Uint64>, Pointer<Uint64>);
// dr_denoise_atrous (the edge-avoiding a-trous filter on the GPU, host buffers; DESIGN.md 2.15): rgb[h][w][3], normal[h][w][3], depth[h][w],
// w, h, DrDenoiseParams (16 bytes, the OFF_DrDenoiseParams_* offsets above), out[h][w][3].  (Signature only, never compiled, like the rest.)
typedef _DenoiseAtrousC = Int32 Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Int32, Int32, Pointer<Uint8>, Pointer<Float>);
typedef _DenoiseAtrousD = int Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, int, int, Pointer<Uint8>, Pointer<Float>);
// dr_denoise_pair (the variance-guided filter on the GPU, host buffers; DESIGN.md 2.19): a[h][w][3], b[h][w][3] -- two renders that differ in the
// sampler's seed alone --, normal[h][w][3], depth[h][w], w, h, DrDenoisePairParams (20 bytes, the OFF_DrDenoisePairParams_* offsets above),
// out[h][w][3], out_var[h][w] or null.  (Signature only, never compiled, like the rest.)
typedef _DenoisePairC = Int32 Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Int32, Int32, Pointer<Uint8>, Pointer<Float>,
    Pointer<Float>);
typedef _DenoisePairD = int Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, int, int, Pointer<Uint8>, Pointer<Float>,
    Pointer<Float>);
// dr_upsample (the joint bilateral upsampler on the GPU, host buffers; DESIGN.md 2.22): rgb_lo[hl][wl][3], normal_lo[hl][wl][3], depth_lo[hl][wl],
// wl, hl, normal[h][w][3], depth[h][w] with w = factor * wl and h = factor * hl, DrUpsampleParams (16 bytes, the OFF_DrUpsampleParams_* offsets
// above), out[h][w][3].  (Signature only, never compiled, like the rest.)
typedef _UpsampleC = Int32 Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Int32, Int32, Pointer<Float>, Pointer<Float>, Pointer<Uint8>,
    Pointer<Float>);
typedef _UpsampleD = int Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, int, int, Pointer<Float>, Pointer<Float>, Pointer<Uint8>,
    Pointer<Float>);
// dr_temporal (temporal accumulation on the GPU, host buffers; DESIGN.md 2.23): rgb[h][w][3], normal[h][w][3], depth[h][w], the history
// h_rgb[h][w][3], h_m2[h][w], h_len[h][w], h_normal[h][w][3], h_depth[h][w] (all five nullptr on the first frame), w, h, DrTemporalParams
// (400 bytes, the OFF_DrTemporalParams_* offsets above), out_rgb[h][w][3], out_m2[h][w], out_len[h][w].  (Signature only, never compiled,
// like the rest.)
typedef _TemporalC = Int32 Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>,
    Pointer<Float>, Int32, Int32, Pointer<Uint8>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _TemporalD = int Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>,
    Pointer<Float>, int, int, Pointer<Uint8>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
// dr_denoise_moments (the variance-guided filter over a temporal history on the GPU, host buffers; DESIGN.md 2.24): what dr_temporal wrote last --
// rgb[h][w][3], m2[h][w], len[h][w] -- and that frame's normal[h][w][3] and depth[h][w], w, h, DrDenoiseMomentsParams (28 bytes, the
// OFF_DrDenoiseMomentsParams_* offsets above), out[h][w][3], out_var[h][w] or null, out_var0[h][w] or null.  (Signature only, never compiled,
// like the rest.)
typedef _DenoiseMomentsC = Int32 Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Int32, Int32,
    Pointer<Uint8>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _DenoiseMomentsD = int Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, Pointer<Float>, int, int, Pointer<Uint8>,
    Pointer<Float>, Pointer<Float>, Pointer<Float>);
// dr_firefly_check (the refusals of the parameters and the size, without an image) and dr_firefly / dr_firefly_host (firefly suppression on
// the GPU and on the host, host buffers; DESIGN.md 2.25): rgb[h][w][3], normal[h][w][3], depth[h][w], w, h, DrFireflyParams (24 bytes, the
// OFF_DrFireflyParams_* offsets above), out[h][w][3], removed[h][w] or null.  dr_firefly_device takes device addresses and a hipStream_t
// last.  (Signatures only, never compiled, like the rest.)
typedef _FireflyCheckC = Int32 Function(Pointer<Uint8>, Int32, Int32);
typedef _FireflyCheckD = int Function(Pointer<Uint8>, int, int);
typedef _FireflyC = Int32 Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Int32, Int32, Pointer<Uint8>, Pointer<Float>, Pointer<Float>);
typedef _FireflyD = int Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, int, int, Pointer<Uint8>, Pointer<Float>, Pointer<Float>);
typedef _FireflyDeviceC = Int32 Function(Pointer<Void>, Pointer<Void>, Pointer<Void>, Int32, Int32, Pointer<Uint8>, Pointer<Void>, Pointer<Void>,
    Pointer<Void>);
typedef _FireflyDeviceD = int Function(Pointer<Void>, Pointer<Void>, Pointer<Void>, int, int, Pointer<Uint8>, Pointer<Void>, Pointer<Void>,
    Pointer<Void>);
// dr_display (the display transform on the GPU, host buffers; DESIGN.md 2.20): rgb[h][w][3], w, h, DrDisplayParams (32 bytes, the
// OFF_DrDisplayParams_* offsets above), out[h][w][4] bytes R, G, B, A.  (Signature only, never compiled, like the rest.)
typedef _DisplayC = Int32 Function(Pointer<Float>, Int32, Int32, Pointer<Uint8>, Pointer<Uint8>);
typedef _DisplayD = int Function(Pointer<Float>, int, int, Pointer<Uint8>, Pointer<Uint8>);
// dr_render_guides_check (the refusals, without a scene or a GPU): DrRenderDesc, DrGuidesDesc (24 bytes, the OFF_DrGuidesDesc_* offsets above),
// the scene's primitive count.  dr_render_guides: dr_render plus, per channel, the address of a film [h*w*4] and (the array or an entry may be
// null) of a resolved image [h*w*3].  dr_render_guides_device: device addresses and a hipStream_t last.  (Signatures only, never compiled,
// like the rest.)
typedef _RenderGuidesCheckC = Int32 Function(Pointer<Uint8>, Pointer<Uint8>, Uint64);
typedef _RenderGuidesCheckD = int Function(Pointer<Uint8>, Pointer<Uint8>, int);
// The two arrays of addresses travel as blocks of 8-byte words (_Blob.addr).
typedef _RenderGuidesC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Pointer<Uint8>, Pointer<Float>, Pointer<Float>, Pointer<Uint8>, Pointer<Uint8>);
typedef _RenderGuidesD = int Function(Pointer<Void>, Pointer<Uint8>, Pointer<Uint8>, Pointer<Float>, Pointer<Float>, Pointer<Uint8>, Pointer<Uint8>);
typedef _RenderGuidesDeviceC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Pointer<Uint8>, Pointer<Void>, Pointer<Uint8>, Pointer<Void>);
typedef _RenderGuidesDeviceD = int Function(Pointer<Void>, Pointer<Uint8>, Pointer<Uint8>, Pointer<Void>, Pointer<Uint8>, Pointer<Void>);
// dr_material_check (what a DR_INTEGRATOR_MATERIAL render of a channel would answer, without a scene or a device)
typedef _MaterialCheckC = Int32 Function(Int32);
typedef _MaterialCheckD = int Function(int);
// dr_demodulate_check, and dr_demodulate / dr_remodulate with their _host forms (DESIGN.md 2.27): rgb[h][w][3], emission[h][w][3] or null,
// albedo[h][w][3] or null, w, h, DrDemodulateParams (4 bytes), out[h][w][3].  The _device forms take device addresses and a hipStream_t
typedef _DemodulateCheckC = Int32 Function(Pointer<Uint8>, Int32, Int32);
typedef _DemodulateCheckD = int Function(Pointer<Uint8>, int, int);
typedef _DemodulateC = Int32 Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, Int32, Int32, Pointer<Uint8>, Pointer<Float>);
typedef _DemodulateD = int Function(Pointer<Float>, Pointer<Float>, Pointer<Float>, int, int, Pointer<Uint8>, Pointer<Float>);
typedef _DemodulateDeviceC = Int32 Function(Pointer<Void>, Pointer<Void>, Pointer<Void>, Int32, Int32, Pointer<Uint8>, Pointer<Void>, Pointer<Void>);
typedef _DemodulateDeviceD = int Function(Pointer<Void>, Pointer<Void>, Pointer<Void>, int, int, Pointer<Uint8>, Pointer<Void>, Pointer<Void>);
typedef _DestroyC = Void Function(Pointer<Void>);
typedef _DestroyD = void Function(Pointer<Void>);
typedef _ErrC = Pointer<Utf8> Function();
typedef _ErrD = Pointer<Utf8> Function();

/// The first-hit feature integrator (DESIGN.md 2.14): the library's own surface integrator, which the reference does not have.  Li is one
/// quantity of the camera ray's Intersection -- channel DR_FEATURE_NG / _NS (0.5 * (normal + 1)), _DEPTH (t, t, t), _UV (u, v, 0) or _ID
/// (primitive + 1, material + 1, 1), and 0 where the ray hits nothing -- a guide image rendered through the same sampler and film as the
/// beauty image.  It exists on the device only (DR_INTEGRATOR_FEATURE, k_shade_feature): the object carries the channel to
/// HipSamplerRenderer, and a host renderer that asks it for Li is told so.
class FeatureIntegrator extends SurfaceIntegrator {
  FeatureIntegrator(this.channel) {
    if (channel < DR_FEATURE_NG || channel > DR_FEATURE_ID) {
      throw new ArgumentError('feature integrator: unknown channel (DR_FEATURE_NG, _NS, _DEPTH, _UV or _ID)');
    }
  }

  Spectrum Li(Scene scene, Renderer renderer, RayDifferential ray, Intersection isect, Sample sample, RNG rng) {
    throw new UnsupportedError('feature integrator: evaluated on the device (HipSamplerRenderer)');
  }

  final int channel;
}

/// The first-hit material integrator (DESIGN.md 2.27), the feature integrator's sibling for what reads a material or a light: Li is channel
/// DR_MATERIAL_CHANNEL_ALBEDO (the camera hit's material colour; 0 at a miss) or _EMISSION (isect.Le(-ray.d) at a hit, the lights' Le(ray) at a
/// miss).  It exists on the device only (DR_INTEGRATOR_MATERIAL, k_shade_material), like FeatureIntegrator.
class MaterialIntegrator extends SurfaceIntegrator {
  MaterialIntegrator(this.channel) {
    if (channel != DR_MATERIAL_CHANNEL_ALBEDO && channel != DR_MATERIAL_CHANNEL_EMISSION) {
      throw new ArgumentError('material integrator: unknown channel (DR_MATERIAL_CHANNEL_ALBEDO or _EMISSION)');
    }
  }

  Spectrum Li(Scene scene, Renderer renderer, RayDifferential ray, Intersection isect, Sample sample, RNG rng) {
    throw new UnsupportedError('material integrator: evaluated on the device (HipSamplerRenderer)');
  }

  final int channel;
}

/// A zero-initialised block of native memory with typed little-endian writers: one per C struct (array).
class _Blob {
  final int length;
  final Pointer<Uint8> ptr;
  ByteData _view;

  _Blob(int bytes)
      : length = bytes < 1 ? 1 : bytes,
        ptr = calloc<Uint8>(bytes < 1 ? 1 : bytes) {
    _view = ByteData.view(ptr.asTypedList(length).buffer, ptr.asTypedList(length).offsetInBytes, length);
  }

  void i32(int off, int v) => _view.setInt32(off, v, Endian.little);
  void u32(int off, int v) => _view.setUint32(off, v, Endian.little);
  void u16(int off, int v) => _view.setUint16(off, v, Endian.little);
  void u8(int off, int v) => _view.setUint8(off, v);
  void i64(int off, int v) => _view.setInt64(off, v, Endian.little);
  void u64(int off, int v) => _view.setUint64(off, v, Endian.little);
  void f32(int off, double v) => _view.setFloat32(off, v, Endian.little);
  void f64(int off, double v) => _view.setFloat64(off, v, Endian.little);
  void addr(int off, _Blob b) => _view.setUint64(off, b == null ? 0 : b.ptr.address, Endian.little);
  void f32s(int off, List<double> v) {
    for (int i = 0; i < v.length; ++i) {
      f32(off + 4 * i, v[i]);
    }
  }

  void free() => calloc.free(ptr);
}

class HipSamplerRenderer extends Renderer {
  static final DynamicLibrary _lib = _open();
  static final _InitD _init = _lib.lookupFunction<_InitC, _InitD>('dr_init');
  /// LoopSubdivision.refine behind the C ABI: the host builder and, after dr_init, the device builder (same bytes).
  static final _LoopSubdivideD loopSubdivide = _lib.lookupFunction<_LoopSubdivideC, _LoopSubdivideD>('dr_loop_subdivide');
  static final _LoopSubdivideD loopSubdivideDevice = _lib.lookupFunction<_LoopSubdivideC, _LoopSubdivideD>('dr_loop_subdivide_device');
  /// Nurbs.refine behind the C ABI: the host builder and, after dr_init, the device builder (same bytes, a NaN's payload aside).
  static final _NurbsDiceD nurbsDice = _lib.lookupFunction<_NurbsDiceC, _NurbsDiceD>('dr_nurbs_dice');
  static final _NurbsDiceD nurbsDiceDevice = _lib.lookupFunction<_NurbsDiceC, _NurbsDiceD>('dr_nurbs_dice_device');
  /// The a-trous denoiser over a finished image and its FeatureIntegrator normal and depth images (after dr_init).
  static final _DenoiseAtrousD denoiseAtrous = _lib.lookupFunction<_DenoiseAtrousC, _DenoiseAtrousD>('dr_denoise_atrous');
  /// The same over two half-sample renders, whose difference estimates the variance that guides the colour term (after dr_init).
  static final _DenoisePairD denoisePair = _lib.lookupFunction<_DenoisePairC, _DenoisePairD>('dr_denoise_pair');
  /// The joint bilateral upsampler: an image rendered at 1/2 or 1/4 of the resolution per axis, brought to the full resolution under
  /// full-resolution FeatureIntegrator normal and depth images (after dr_init).
  static final _UpsampleD upsample = _lib.lookupFunction<_UpsampleC, _UpsampleD>('dr_upsample');
  /// Temporal accumulation: one frame of a camera animation blended into the history of the frames before it, where the previous frame
  /// saw the same surface (after dr_init).  The host composes the three matrices of DrTemporalParams from the two cameras.
  static final _TemporalD temporal = _lib.lookupFunction<_TemporalC, _TemporalD>('dr_temporal');
  /// The variance-guided a-trous denoiser over what `temporal` wrote last: the history's luminance moments give the per-pixel variance
  /// that guides the colour term (after dr_init).
  static final _DenoiseMomentsD denoiseMoments = _lib.lookupFunction<_DenoiseMomentsC, _DenoiseMomentsD>('dr_denoise_moments');
  /// Firefly suppression: a pixel far brighter than its same-surface neighbours is scaled down to their level, ahead of `temporal` and
  /// the denoisers (`firefly` and `fireflyDevice` after dr_init; `fireflyHost` and `fireflyCheck` need no GPU).
  static final _FireflyCheckD fireflyCheck = _lib.lookupFunction<_FireflyCheckC, _FireflyCheckD>('dr_firefly_check');
  static final _FireflyD fireflyHost = _lib.lookupFunction<_FireflyC, _FireflyD>('dr_firefly_host');
  static final _FireflyD firefly = _lib.lookupFunction<_FireflyC, _FireflyD>('dr_firefly');
  static final _FireflyDeviceD fireflyDevice = _lib.lookupFunction<_FireflyDeviceC, _FireflyDeviceD>('dr_firefly_device');
  /// Demodulation: the emission and albedo images of MaterialIntegrator are taken out of the beauty image ahead of every other image stage
  /// (`demodulate`) and put back after the last (`remodulate`); the `Device` forms after dr_init, the `Host` forms and the checks without a GPU.
  static final _MaterialCheckD materialCheck = _lib.lookupFunction<_MaterialCheckC, _MaterialCheckD>('dr_material_check');
  static final _DemodulateCheckD demodulateCheck = _lib.lookupFunction<_DemodulateCheckC, _DemodulateCheckD>('dr_demodulate_check');
  static final _DemodulateD demodulateHost = _lib.lookupFunction<_DemodulateC, _DemodulateD>('dr_demodulate_host');
  static final _DemodulateD demodulate = _lib.lookupFunction<_DemodulateC, _DemodulateD>('dr_demodulate');
  static final _DemodulateDeviceD demodulateDevice = _lib.lookupFunction<_DemodulateDeviceC, _DemodulateDeviceD>('dr_demodulate_device');
  static final _DemodulateD remodulateHost = _lib.lookupFunction<_DemodulateC, _DemodulateD>('dr_remodulate_host');
  static final _DemodulateD remodulate = _lib.lookupFunction<_DemodulateC, _DemodulateD>('dr_remodulate');
  static final _DemodulateDeviceD remodulateDevice = _lib.lookupFunction<_DemodulateDeviceC, _DemodulateDeviceD>('dr_remodulate_device');
  /// The display transform: linear f32 radiance to RGBA8 through exposure, a tone curve and an 8-bit encode (after dr_init).
  static final _DisplayD displayImage = _lib.lookupFunction<_DisplayC, _DisplayD>('dr_display');
  /// DR_ABI_VERSION of the include/dartray_hip.h these offsets were written against: the structs carry no size field, so a
  /// library of another layout version is refused before any struct crosses the boundary.
  static const int ABI_VERSION = 9;
  static DynamicLibrary _open() {
    DynamicLibrary l = DynamicLibrary.open('libdartray_hip.so');
    _CommVoidD abi = l.lookupFunction<_CommVoidC, _CommVoidD>('dr_abi_version');
    if (abi() != ABI_VERSION) {
      String msg = 'libdartray_hip.so has ABI version ${abi()}, this binding was written against $ABI_VERSION';
      LogSevere(msg);
      throw new StateError(msg);  // (a logger installed by the host need not throw: log.dart:42-47 is the default's behaviour)
    }
    return l;
  }
  static final _SceneCreateD _sceneCreate = _lib.lookupFunction<_SceneCreateC, _SceneCreateD>('dr_scene_create');
  static final _RenderD _render = _lib.lookupFunction<_RenderC, _RenderD>('dr_render');
  /// The guide images of the denoisers in the beauty render's own pass (DESIGN.md 2.26): `renderGuidesCheck` needs no GPU;
  /// `renderGuidesDevice` is `renderDevice`'s twin for hosts that keep the films on the device.
  static final _RenderGuidesCheckD renderGuidesCheck =
      _lib.lookupFunction<_RenderGuidesCheckC, _RenderGuidesCheckD>('dr_render_guides_check');
  static final _RenderGuidesD _renderGuides = _lib.lookupFunction<_RenderGuidesC, _RenderGuidesD>('dr_render_guides');
  static final _RenderGuidesDeviceD renderGuidesDevice =
      _lib.lookupFunction<_RenderGuidesDeviceC, _RenderGuidesDeviceD>('dr_render_guides_device');
  static final _DestroyD _destroy = _lib.lookupFunction<_DestroyC, _DestroyD>('dr_scene_destroy');
  // the multi-GPU half (include/dartray_hip.h): one process per GPU, ONE film reduce per render
  static final _RenderShardedD _renderSharded = _lib.lookupFunction<_RenderShardedC, _RenderShardedD>('dr_render_sharded');
  static final _CommIdD _commUniqueId = _lib.lookupFunction<_CommIdC, _CommIdD>('dr_comm_unique_id');
  static final _CommInitD _commInit = _lib.lookupFunction<_CommInitC, _CommInitD>('dr_comm_init');
  static final _CommVoidD _commDestroy = _lib.lookupFunction<_CommVoidC, _CommVoidD>('dr_comm_destroy');
  static final _CommVoidD _commWorld = _lib.lookupFunction<_CommVoidC, _CommVoidD>('dr_comm_world');
  static final _CommVoidD _commRank = _lib.lookupFunction<_CommVoidC, _CommVoidD>('dr_comm_rank');
  static final _CommVoidD _commAvailable = _lib.lookupFunction<_CommVoidC, _CommVoidD>('dr_comm_available');
  static final _SetOptionD _setOption = _lib.lookupFunction<_SetOptionC, _SetOptionD>('dr_set_option');
  static final _SetGlossyPrtD _setGlossyPrt = _lib.lookupFunction<_SetGlossyPrtC, _SetGlossyPrtD>('dr_scene_set_glossy_prt');
  static final _SetProbesD setProbes = _lib.lookupFunction<_SetProbesC, _SetProbesD>('dr_scene_set_probes');
  static final _ProbesBakeD probesBake = _lib.lookupFunction<_ProbesBakeC, _ProbesBakeD>('dr_probes_bake');
  static final _ProbesGridD probesGrid = _lib.lookupFunction<_ProbesGridC, _ProbesGridD>('dr_probes_grid');
  static final _ProbesPointsD probesSurfacePoints = _lib.lookupFunction<_ProbesPointsC, _ProbesPointsD>('dr_probes_surface_points');
  static final _ProbesCandidatesD probesCandidates = _lib.lookupFunction<_ProbesCandidatesC, _ProbesCandidatesD>('dr_probes_candidates');
  static final _SetLayoutD _setStateLayout = _lib.lookupFunction<_SetLayoutC, _SetLayoutD>('dr_scene_set_state_layout');
  static final _GetLayoutD _getStateLayout = _lib.lookupFunction<_GetLayoutC, _GetLayoutD>('dr_scene_get_state_layout');
  static final _KernelsD _getTraceKernels = _lib.lookupFunction<_KernelsC, _KernelsD>('dr_scene_get_trace_kernels');
  static final _KernelsD _setTraceKernels = _lib.lookupFunction<_KernelsC, _KernelsD>('dr_scene_set_trace_kernels');
  static final _AdaptivePixelsD _getAdaptivePixels =
      _lib.lookupFunction<_AdaptivePixelsC, _AdaptivePixelsD>('dr_scene_get_adaptive_pixels');

  static final _HaltonSamplesD _generateHaltonSamples =
      _lib.lookupFunction<_HaltonSamplesC, _HaltonSamplesD>('dr_generate_halton_samples');

  /// Diagnostics (dr_generate_halton_samples): how many of the indices [first, first + count) of a Halton render's sequence fall inside
  /// the task's window.  [rd] is the render descriptor as render() fills it, [stride] the floats of a sample vector.
  int _haltonAccepted(Pointer<Void> scene, _Blob rd, int first, int count, int stride) {
    Pointer<Uint64> indices = calloc<Uint64>(count < 1 ? 1 : count);
    Pointer<Int32> pixels = calloc<Int32>(count < 1 ? 2 : 2 * count);
    Pointer<Float> vectors = calloc<Float>(count < 1 ? 1 : count * stride);
    Pointer<Uint64> accepted = calloc<Uint64>(1);
    try {
      _check(_generateHaltonSamples(scene, rd.ptr, first, count, indices, pixels, vectors, stride, accepted));
      return accepted.value;
    } finally {
      calloc.free(indices);
      calloc.free(pixels);
      calloc.free(vectors);
      calloc.free(accepted);
    }
  }

  /// How many pixels the last render of this renderer traced a second time at the adaptive sampler's maximum count
  /// (dr_scene_get_adaptive_pixels; 0 under every other sampler).
  int lastSupersampledPixels = 0;

  void _readSupersampled(Pointer<Void> scene) {
    Pointer<Uint64> count = calloc<Uint64>(1);
    try {
      _check(_getAdaptivePixels(scene, nullptr, 0, count));
      lastSupersampledPixels = count.value;
    } finally {
      calloc.free(count);
    }
  }

  /// What the library's pilot picked for a scene: [closest-hit kernel, any-hit kernel, state layout] (include/dartray_hip.h:
  /// dr_scene_get_trace_kernels / dr_scene_get_state_layout).  A render of a big scene measures them on its first batches; a host
  /// that renders the same scene again (animation frames: this renderer builds a device scene per render, like the reference's
  /// isolates load the scene per task) or a manager that knows rank 0's picks hands them in through [pilotPicks] and the render
  /// runs no calibration batches -- and, on N GPUs, every rank runs the same kernels (a step is the slowest rank's: the Python
  /// host's dartray_amd/dist.py share_pilot does the same over its control plane).  Every kernel and layout is bit-exact: the
  /// image does not depend on them.  [lastPilotPicks] is what the last render of this renderer ended up with.
  List<int> pilotPicks;
  List<int> lastPilotPicks;

  void _applyPilotPicks(Pointer<Void> scene) {
    if (pilotPicks == null || pilotPicks.length != 3) {
      return;
    }
    if (pilotPicks[0] != 0 && pilotPicks[1] != 0) {
      Pointer<Uint32> k = calloc<Uint32>(2);
      try {
        k[0] = pilotPicks[0];
        k[1] = pilotPicks[1];
        _check(_setTraceKernels(scene, k));
      } finally {
        calloc.free(k);
      }
    }
    if (pilotPicks[2] != 0) {
      _check(_setStateLayout(scene, pilotPicks[2]));
    }
  }

  void _readPilotPicks(Pointer<Void> scene) {
    Pointer<Uint32> k = calloc<Uint32>(2);
    Pointer<Int32> lay = calloc<Int32>(1);
    try {
      _check(_getTraceKernels(scene, k));
      _check(_getStateLayout(scene, lay, nullptr));
      lastPilotPicks = [k[0], k[1], lay[0]];
    } finally {
      calloc.free(k);
      calloc.free(lay);
    }
  }

  /// Can this process join a multi-GPU render?  Binds librccl and checks its version WITHOUT talking to another rank, so
  /// that the workers can agree on it before anyone blocks in [commInit] (hip_render_manager.dart).
  static bool commAvailable(int device) {
    _checkStatic(_init(device));
    return _commAvailable() == 0;
  }

  /// A tuning / diagnostic switch of the library (the DARTRAY_* names of include/dartray_hip.h, without setenv): read
  /// at every use, so it applies from the next render on; value null returns the switch to the environment's value.
  static void setOption(String name, String value) {
    Pointer<Utf8> n = name.toNativeUtf8();
    Pointer<Utf8> v = value == null ? nullptr : value.toNativeUtf8();
    try {
      _checkStatic(_setOption(n, v));
    } finally {
      calloc.free(n);
      if (v != nullptr) calloc.free(v);
    }
  }
  // for hosts that keep the film on the device themselves (device pointers come from their own HIP binding)
  static final _RenderDeviceD renderDevice = _lib.lookupFunction<_RenderDeviceC, _RenderDeviceD>('dr_render_device');
  static final _FilmReduceD filmReduce = _lib.lookupFunction<_FilmReduceC, _FilmReduceD>('dr_film_reduce');
  static final _FilmResolveD filmResolveDevice = _lib.lookupFunction<_FilmResolveC, _FilmResolveD>('dr_film_resolve_device');

  /// Rank 0 of a multi-GPU render: the 128 opaque bytes every other rank needs for [commInit] (carried by the host:
  /// a file, a pipe, a socket -- hip_render_manager.dart uses a file).
  static Uint8List commUniqueId(int device) {
    _checkStatic(_init(device));
    Pointer<Uint8> id = calloc<Uint8>(DR_COMM_ID_BYTES);
    try {
      _checkStatic(_commUniqueId(id, DR_COMM_ID_BYTES));
      return new Uint8List.fromList(id.asTypedList(DR_COMM_ID_BYTES));
    } finally {
      calloc.free(id);
    }
  }

  /// Every rank, once, after dr_init(device): joins the RCCL communicator of `world` ranks.
  static void commInit(int device, int rank, int world, Uint8List id) {
    _checkStatic(_init(device));
    Pointer<Uint8> p = calloc<Uint8>(DR_COMM_ID_BYTES);
    try {
      p.asTypedList(DR_COMM_ID_BYTES).setAll(0, id);
      _checkStatic(_commInit(rank, world, p, DR_COMM_ID_BYTES));
    } finally {
      calloc.free(p);
    }
  }

  static void commDestroy() => _checkStatic(_commDestroy());

  static void _checkStatic(int rc) {
    if (rc != 0) {
      LogSevere('dartray_hip error $rc: ${_err().toDartString()}');
    }
  }
  static final _ErrD _err = _lib.lookupFunction<_ErrC, _ErrD>('dr_last_error');

  /// tileRank / tileCount: this process's share of the image's 32 x 32 tiles (round-robin) when a render is spread
  /// over several GPUs (one process each, see hip_render_manager.dart); the default is the whole image.
  HipSamplerRenderer(this.sampler, this.camera, this.surfaceIntegrator, this.volumeIntegrator,
                     [this.taskNum = 0, this.taskCount = 1, this.device = 0, this.seed = 5489,
                      this.tileRank = 0, this.tileCount = 1]);

  /// Every failure of the library becomes a LogSevere, i.e. an Exception (log.dart:42-47), which
  /// DartRay.worldEnd turns into completeError (dartray.dart:573-583).
  void _check(int rc) {
    if (rc != 0) {
      LogSevere('dartray_hip error $rc: ${_err().toDartString()}');
    }
  }

  static void _unsupported(String what) {
    LogSevere('HipSamplerRenderer: $what is outside the device path');
  }

  static List<double> _rgb(Spectrum s) {
    RGBColor c = s.toRGB();
    return [c.c[0], c.c[1], c.c[2]];
  }

  /// Kd / Kr / Kt / sigma / index are Textures; the device path takes constants (evaluate() of a constant texture
  /// ignores the DifferentialGeometry).
  static final DifferentialGeometry _dg0 = new DifferentialGeometry();

  /// render(), and in the same pass the FeatureIntegrator images of [channels] (DR_FEATURE_* values, at most five, none twice): the
  /// OutputImage of render(); the guides stay in [lastGuides], one [height * width * 3] image per channel in the order given.  Path,
  /// DirectLighting, Whitted and ambient occlusion integrators, one process (tileCount 1); the library refuses everything else by name.
  Future<OutputImage> renderWithGuides(Scene scene, List<int> channels) {
    _guideChannels = channels;
    lastGuides = null;
    try {
      return render(scene);
    } finally {
      _guideChannels = null;
    }
  }

  /// The guide images of the last renderWithGuides call (null after a plain render).
  List<Float32List> lastGuides;
  List<int> _guideChannels;

  Future<OutputImage> render(Scene scene) {
    Completer<OutputImage> completer = new Completer<OutputImage>();
    List<_Blob> blobs = [];
    Pointer<Pointer<Void>> handle = calloc<Pointer<Void>>();
    Pointer<Float> lxyzw = nullptr;
    Pointer<Float> rgb = nullptr;
    try {
      _check(_init(device));
      if (scene.aggregate is! BVHAccel) {
        _unsupported('aggregate ${scene.aggregate.runtimeType} (only "bvh")');
      }
      if (scene.volumeRegion != null) {
        _unsupported('a VolumeRegion');
      }
      BVHAccel bvh = scene.aggregate;

      // ---- BVHAccel.nodes: _LinearBVHNode { bounds, offset, nPrimitives, axis } (bvh_accel.dart:533-538) ----
      final int nnodes = bvh.nodes == null ? 0 : bvh.nodes.length;
      _Blob nodes = new _Blob(nnodes * SIZEOF_DrBvhNode);
      blobs.add(nodes);
      for (int i = 0; i < nnodes; ++i) {
        var n = bvh.nodes[i];
        int o = i * SIZEOF_DrBvhNode;
        nodes.f32s(o + OFF_DrBvhNode_bmin, [n.bounds.pMin.x, n.bounds.pMin.y, n.bounds.pMin.z]);
        nodes.f32s(o + OFF_DrBvhNode_bmax, [n.bounds.pMax.x, n.bounds.pMax.y, n.bounds.pMax.z]);
        nodes.u32(o + OFF_DrBvhNode_offset, n.offset);
        nodes.u16(o + OFF_DrBvhNode_nprims, n.nPrimitives);
        nodes.u8(o + OFF_DrBvhNode_axis, n.nPrimitives > 0 ? 0 : n.axis);
      }

      // ---- BVHAccel.primitives, in BVH order: shapes, materials, area lights ----
      final int nprims = bvh.primitives.length;
      Map<TriangleMesh, int> meshBase = {};      // first vertex of each mesh in the shared vertex array
      List<TriangleMesh> meshes = [];
      int nverts = 0;
      List<Shape> quadrics = [];
      Map<Shape, int> quadricIndex = {};
      List<Material> materials = [];
      Map<Material, int> materialIndex = {};
      Map<Light, int> lightIndex = {};
      for (int i = 0; i < scene.lights.length; ++i) {
        lightIndex[scene.lights[i]] = i;
      }
      int baseOf(TriangleMesh m) {
        if (!meshBase.containsKey(m)) {
          meshBase[m] = nverts;
          meshes.add(m);
          nverts += m.nverts;
        }
        return meshBase[m];
      }
      int quadricOf(Shape s) {
        if (!quadricIndex.containsKey(s)) {
          quadricIndex[s] = quadrics.length;
          quadrics.add(s);
        }
        return quadricIndex[s];
      }

      _Blob triIdx = new _Blob(nprims * 12);
      _Blob triMaterial = new _Blob(nprims * 4);
      _Blob triLight = new _Blob(nprims * 4);
      _Blob triReverse = new _Blob(nprims);
      _Blob triShading = new _Blob(nprims);
      _Blob triXform = new _Blob(nprims * 4);
      bool anyShading = false;
      List<TriangleMesh> xformMeshes = [];
      Map<TriangleMesh, int> xformIndex = {};
      blobs.addAll([triIdx, triMaterial, triLight, triReverse, triShading, triXform]);
      for (int i = 0; i < nprims; ++i) {
        if (bvh.primitives[i] is! GeometricPrimitive) {
          _unsupported('primitive ${bvh.primitives[i].runtimeType} (instancing)');
        }
        GeometricPrimitive gp = bvh.primitives[i];
        Shape sh = gp.shape;
        if (sh is Triangle) {
          if (sh.mesh.alphaTexture != null) {
            _unsupported('an alpha texture');
          }
          int b = baseOf(sh.mesh);
          // per-vertex N / S / uv (triangle_mesh.dart:195-203): which attributes the primitive's mesh has, and the
          // mesh transform that takes N / S to world space at shading time (triangle.dart:303-317)
          int bits = (sh.mesh.n != null ? DR_SHADING_N : 0) | (sh.mesh.s != null ? DR_SHADING_S : 0) |
                     (sh.mesh.uvs != null ? DR_SHADING_UV : 0);
          triShading.u8(i, bits);
          if (bits != 0) {
            anyShading = true;
          }
          if ((bits & (DR_SHADING_N | DR_SHADING_S)) != 0) {
            if (!xformIndex.containsKey(sh.mesh)) {
              xformIndex[sh.mesh] = xformMeshes.length;
              xformMeshes.add(sh.mesh);
            }
            triXform.u32(4 * i, xformIndex[sh.mesh]);
          }
          for (int k = 0; k < 3; ++k) {
            triIdx.u32(12 * i + 4 * k, b + sh.mesh.vertexIndex[sh.index + k]);   // Triangle.v(k) (triangle.dart:241)
          }
        } else if (sh is Sphere || sh is Disk) {
          triIdx.u32(12 * i, DR_PRIM_QUADRIC);
          triIdx.u32(12 * i + 4, quadricOf(sh));
        } else {
          _unsupported('shape ${sh.runtimeType}');
        }
        if (!materialIndex.containsKey(gp.material)) {
          materialIndex[gp.material] = materials.length;
          materials.add(gp.material);
        }
        triMaterial.u32(4 * i, materialIndex[gp.material]);
        triLight.i32(4 * i, gp.areaLight == null ? -1 : lightIndex[gp.areaLight]);
        triReverse.u8(i, sh.reverseOrientation ? 1 : 0);
      }

      // world-space vertices: TriangleMesh.point(i) (triangle_mesh.dart:39-42)
      _Blob verts = new _Blob(nverts * 12);
      blobs.add(verts);
      for (TriangleMesh m in meshes) {
        int b = meshBase[m];
        for (int i = 0; i < m.nverts; ++i) {
          Point p = m.point(i);
          verts.f32s(12 * (b + i), [p.x, p.y, p.z]);
        }
      }

      // per-vertex normals / tangents (OBJECT space: TriangleMesh keeps them as given) and uvs, indexed like verts
      _Blob vertN, vertS, vertUV, meshXforms;
      if (anyShading) {
        vertN = new _Blob(nverts * 12);
        vertS = new _Blob(nverts * 12);
        vertUV = new _Blob(nverts * 8);
        meshXforms = new _Blob(xformMeshes.length * SIZEOF_DrMeshXform);
        blobs.addAll([vertN, vertS, vertUV, meshXforms]);
        for (TriangleMesh m in meshes) {
          int b = meshBase[m];
          for (int i = 0; i < m.nverts; ++i) {
            if (m.n != null) {
              vertN.f32s(12 * (b + i), [m.n[i].x, m.n[i].y, m.n[i].z]);
            }
            if (m.s != null) {
              vertS.f32s(12 * (b + i), [m.s[i].x, m.s[i].y, m.s[i].z]);
            }
            if (m.uvs != null) {
              vertUV.f32s(8 * (b + i), [m.uvs[2 * i], m.uvs[2 * i + 1]]);
            }
          }
        }
        for (int i = 0; i < xformMeshes.length; ++i) {
          meshXforms.f32s(i * SIZEOF_DrMeshXform + OFF_DrMeshXform_object_to_world, xformMeshes[i].objectToWorld.m.data);
          meshXforms.f32s(i * SIZEOF_DrMeshXform + OFF_DrMeshXform_world_to_object, xformMeshes[i].worldToObject.m.data);
        }
      }

      // quadrics: constructor arguments as the Dart doubles they are (sphere.dart:313-321, disk.dart:157-165)
      _Blob quads = new _Blob(quadrics.length * SIZEOF_DrQuadric);
      blobs.add(quads);
      for (int i = 0; i < quadrics.length; ++i) {
        Shape s = quadrics[i];
        int o = i * SIZEOF_DrQuadric;
        quads.f32s(o + OFF_DrQuadric_object_to_world, s.objectToWorld.m.data);
        quads.f32s(o + OFF_DrQuadric_world_to_object, s.worldToObject.m.data);
        if (s is Sphere) {
          quads.i32(o + OFF_DrQuadric_kind, DR_QUADRIC_SPHERE);
          // (phiMax is stored in radians, sphere.dart:313-321: Degrees(Radians(x)) is x up to an ulp, exact for 360)
          List<double> p = [s.radius, s.zmin, s.zmax, Degrees(s.phiMax)];
          for (int k = 0; k < 4; ++k) {
            quads.f64(o + OFF_DrQuadric_params + 8 * k, p[k]);
          }
        } else if (s is Disk) {
          quads.i32(o + OFF_DrQuadric_kind, DR_QUADRIC_DISK);
          List<double> p = [s.height, s.radius, s.innerRadius, Degrees(s.phiMax)];
          for (int k = 0; k < 4; ++k) {
            quads.f64(o + OFF_DrQuadric_params + 8 * k, p[k]);
          }
        }
      }

      // ---- materials with constant textures ----
      _Blob mats = new _Blob(materials.length * SIZEOF_DrMaterial);
      blobs.add(mats);
      for (int i = 0; i < materials.length; ++i) {
        Material m = materials[i];
        int o = i * SIZEOF_DrMaterial;
        if (m is MatteMaterial) {                         // matte_material.dart:41-65
          if (m.bumpMap != null) {
            _unsupported('a bump map');
          }
          mats.i32(o + OFF_DrMaterial_type, DR_MATERIAL_MATTE);
          mats.f32s(o + OFF_DrMaterial_kd, _rgb(m.Kd.evaluate(_dg0)));
          mats.f64(o + OFF_DrMaterial_sigma, m.sigma.evaluate(_dg0));
        } else if (m is MirrorMaterial) {                 // mirror_material.dart:38-55
          mats.i32(o + OFF_DrMaterial_type, DR_MATERIAL_MIRROR);
          mats.f32s(o + OFF_DrMaterial_kr, _rgb(m.Kr.evaluate(_dg0)));
        } else if (m is GlassMaterial) {                  // glass_material.dart:44-69
          mats.i32(o + OFF_DrMaterial_type, DR_MATERIAL_GLASS);
          mats.f32s(o + OFF_DrMaterial_kr, _rgb(m.Kr.evaluate(_dg0)));
          mats.f32s(o + OFF_DrMaterial_kt, _rgb(m.Kt.evaluate(_dg0)));
          mats.f64(o + OFF_DrMaterial_index, m.index.evaluate(_dg0));
        } else if (m is PlasticMaterial) {                // plastic_material.dart:43-70
          mats.i32(o + OFF_DrMaterial_type, DR_MATERIAL_PLASTIC);
          mats.f32s(o + OFF_DrMaterial_kd, _rgb(m.Kd.evaluate(_dg0)));
          mats.f32s(o + OFF_DrMaterial_kr, _rgb(m.Ks.evaluate(_dg0)));
          mats.f64(o + OFF_DrMaterial_index, m.roughness.evaluate(_dg0));
        } else {
          _unsupported('material ${m.runtimeType}');
        }
      }

      // ---- scene.lights, in list order (the order lightNum indexes) ----
      final int nlights = scene.lights.length;
      _Blob lights = new _Blob(nlights * SIZEOF_DrAreaLight);
      blobs.add(lights);
      List<List<int>> lightTris = [];   // (v0, v1, v2, reverse) or (DR_PRIM_QUADRIC, quadric, 0, reverse)
      _Blob envMaps;
      _Blob envTexels;
      for (int i = 0; i < nlights; ++i) {
        Light l = scene.lights[i];
        int o = i * SIZEOF_DrAreaLight;
        if (l is DiffuseAreaLight) {                      // diffuse_area_light.dart:36-43
          lights.u32(o + OFF_DrAreaLight_kind, DR_LIGHT_DIFFUSE_AREA);
          lights.f32s(o + OFF_DrAreaLight_L, _rgb(l.Lemit));
          lights.i32(o + OFF_DrAreaLight_nsamples, l.nSamples);
          lights.u32(o + OFF_DrAreaLight_first_tri, lightTris.length);
          for (Shape s in l.shapeSet.shapes) {            // ShapeSet order: the LIFO refine order (shape_set.dart:27-35)
            if (s is Triangle) {
              int b = baseOf(s.mesh);                     // (an emitter's mesh is also a primitive's mesh: already placed)
              // bit 1: the mesh has uvs -- they decide dpdu x dpdv, i.e. the side the emitter shines from
              lightTris.add([b + s.mesh.vertexIndex[s.index], b + s.mesh.vertexIndex[s.index + 1],
                             b + s.mesh.vertexIndex[s.index + 2],
                             (s.reverseOrientation ? 1 : 0) | (s.mesh.uvs != null ? 2 : 0)]);
            } else if (s is Sphere || s is Disk) {
              lightTris.add([DR_PRIM_QUADRIC, quadricOf(s), 0, s.reverseOrientation ? 1 : 0]);
            } else {
              _unsupported('emissive shape ${s.runtimeType}');
            }
          }
          lights.u32(o + OFF_DrAreaLight_ntris, lightTris.length - lights._view.getUint32(o + OFF_DrAreaLight_first_tri, Endian.little));
        } else if (l is InfiniteAreaLight) {              // infinite_area_light.dart
          if (envMaps != null) {
            _unsupported('more than one infinite light');
          }
          lights.u32(o + OFF_DrAreaLight_kind, DR_LIGHT_INFINITE);
          lights.f32s(o + OFF_DrAreaLight_L, _rgb(l.L));
          lights.i32(o + OFF_DrAreaLight_nsamples, l.nSamples);
          lights.u32(o + OFF_DrAreaLight_env_index, 0);
          // level 0 of the radiance MIPMap (mipmap.dart:139): width x height RGB texels
          final int w = l.radianceMap.width, h = l.radianceMap.height;
          envTexels = new _Blob(w * h * 12);
          for (int t = 0; t < h; ++t) {
            for (int s = 0; s < w; ++s) {
              envTexels.f32s(12 * (t * w + s), _rgb(l.radianceMap.texel(0, s, t)));
            }
          }
          envMaps = new _Blob(SIZEOF_DrEnvMap);
          envMaps.addr(OFF_DrEnvMap_texels, envTexels);
          envMaps.i32(OFF_DrEnvMap_width, w);
          envMaps.i32(OFF_DrEnvMap_height, h);
          envMaps.f32s(OFF_DrEnvMap_light_to_world, l.lightToWorld.m.data);
          envMaps.f32s(OFF_DrEnvMap_world_to_light, l.worldToLight.m.data);
          blobs.addAll([envTexels, envMaps]);
        } else if (l is SpotLight) {
          // A constructed SpotLight only keeps the two cosines (spot_light.dart:46-47); DR_LIGHT_SPOT_COS takes
          // exactly those doubles (DR_LIGHT_SPOT takes the constructor's degrees).  SpotLight extends Light, not
          // PointLight: this branch precedes the PointLight one only for readability.
          lights.u32(o + OFF_DrAreaLight_kind, DR_LIGHT_SPOT_COS);
          lights.f32s(o + OFF_DrAreaLight_L, _rgb(l.intensity));
          lights.i32(o + OFF_DrAreaLight_nsamples, 1);
          lights.f32s(o + OFF_DrAreaLight_position, [l.lightPos.x, l.lightPos.y, l.lightPos.z]);
          lights.f32s(o + OFF_DrAreaLight_world_to_light, l.worldToLight.m.data);
          lights.f64(o + OFF_DrAreaLight_cone_width, l.cosTotalWidth);
          lights.f64(o + OFF_DrAreaLight_cone_falloff_start, l.cosFalloffStart);
        } else if (l is PointLight) {                     // point_light.dart:36-39
          lights.u32(o + OFF_DrAreaLight_kind, DR_LIGHT_POINT);
          lights.f32s(o + OFF_DrAreaLight_L, _rgb(l.intensity));
          lights.i32(o + OFF_DrAreaLight_nsamples, 1);
          lights.f32s(o + OFF_DrAreaLight_position, [l.lightPos.x, l.lightPos.y, l.lightPos.z]);
        } else if (l is DistantLight) {                   // distant_light.dart:38-42
          lights.u32(o + OFF_DrAreaLight_kind, DR_LIGHT_DISTANT);
          lights.f32s(o + OFF_DrAreaLight_L, _rgb(l.L));
          lights.i32(o + OFF_DrAreaLight_nsamples, 1);
          lights.f32s(o + OFF_DrAreaLight_position, [l.lightDir.x, l.lightDir.y, l.lightDir.z]);
        } else {
          _unsupported('light ${l.runtimeType}');
        }
      }
      _Blob ltris = new _Blob(lightTris.length * SIZEOF_DrLightTri);
      blobs.add(ltris);
      for (int i = 0; i < lightTris.length; ++i) {
        for (int k = 0; k < 4; ++k) {
          ltris.u32(i * SIZEOF_DrLightTri + 4 * k, lightTris[i][k]);
        }
      }

      // ---- DrSceneDesc ----
      _Blob sd = new _Blob(SIZEOF_DrSceneDesc);
      blobs.add(sd);
      sd.addr(OFF_DrSceneDesc_nodes, nodes);
      sd.u64(OFF_DrSceneDesc_nnodes, nnodes);
      sd.addr(OFF_DrSceneDesc_verts, verts);
      sd.u64(OFF_DrSceneDesc_nverts, nverts);
      sd.addr(OFF_DrSceneDesc_tri_idx, triIdx);
      sd.u64(OFF_DrSceneDesc_ntris, nprims);
      sd.addr(OFF_DrSceneDesc_tri_material, triMaterial);
      sd.addr(OFF_DrSceneDesc_tri_light, triLight);
      sd.addr(OFF_DrSceneDesc_tri_reverse, triReverse);
      sd.addr(OFF_DrSceneDesc_materials, mats);
      sd.u32(OFF_DrSceneDesc_nmaterials, materials.length);
      sd.addr(OFF_DrSceneDesc_lights, lights);
      sd.u32(OFF_DrSceneDesc_nlights, nlights);
      sd.addr(OFF_DrSceneDesc_light_tris, ltris);
      sd.u32(OFF_DrSceneDesc_nlight_tris, lightTris.length);
      sd.u32(OFF_DrSceneDesc_bvh_depth, 0);               // a Dart BVHAccel does not record its depth: the library measures it
      sd.addr(OFF_DrSceneDesc_env_maps, envMaps);
      sd.u32(OFF_DrSceneDesc_nenv_maps, envMaps == null ? 0 : 1);
      sd.addr(OFF_DrSceneDesc_quadrics, quads);
      sd.u32(OFF_DrSceneDesc_nquadrics, quadrics.length);
      if (anyShading) {
        sd.addr(OFF_DrSceneDesc_vert_normals, vertN);
        sd.addr(OFF_DrSceneDesc_vert_tangents, vertS);
        sd.addr(OFF_DrSceneDesc_vert_uvs, vertUV);
        sd.addr(OFF_DrSceneDesc_tri_shading, triShading);
        sd.addr(OFF_DrSceneDesc_tri_xform, triXform);
        sd.addr(OFF_DrSceneDesc_mesh_xforms, meshXforms);
        sd.u32(OFF_DrSceneDesc_nmesh_xforms, xformMeshes.length);
      }
      _check(_sceneCreate(sd.ptr, handle));
      _applyPilotPicks(handle.value);

      // ---- DrRenderDesc: camera, film, integrator, sampler, task (sampler_renderer.dart:29-31,36-65) ----
      _Blob rd = new _Blob(SIZEOF_DrRenderDesc);
      blobs.add(rd);
      int cam = OFF_DrRenderDesc_camera;
      rd.f32s(cam + OFF_DrCamera_camera_to_world, camera.cameraToWorld.startTransform.m.data);
      rd.f64(cam + OFF_DrCamera_shutter_open, camera.shutterOpen);
      rd.f64(cam + OFF_DrCamera_shutter_close, camera.shutterClose);
      if (camera is PerspectiveCamera || camera is OrthographicCamera) {
        ProjectiveCamera pc = camera;
        rd.f32s(cam + OFF_DrCamera_raster_to_camera, pc.rasterToCamera.m.data);
        rd.f64(cam + OFF_DrCamera_lens_radius, pc.lensRadius);
        rd.f64(cam + OFF_DrCamera_focal_distance, pc.focalDistance);
        rd.i32(cam + OFF_DrCamera_type, camera is PerspectiveCamera ? DR_CAMERA_PERSPECTIVE : DR_CAMERA_ORTHOGRAPHIC);
      } else if (camera is EnvironmentCamera) {
        rd.i32(cam + OFF_DrCamera_type, DR_CAMERA_ENVIRONMENT);
      } else {
        _unsupported('camera ${camera.runtimeType}');
      }
      if (camera.film is! ImageFilm) {
        _unsupported('film ${camera.film.runtimeType}');
      }
      ImageFilm film = camera.film;
      int fo = OFF_DrRenderDesc_film;
      rd.i32(fo + OFF_DrFilm_xres, film.xResolution);
      rd.i32(fo + OFF_DrFilm_yres, film.yResolution);
      for (int k = 0; k < 4; ++k) {
        rd.f64(fo + OFF_DrFilm_crop + 8 * k, film.cropWindow[k]);
      }
      rd.f64(fo + OFF_DrFilm_filter_xw, film.filter.xWidth);
      rd.f64(fo + OFF_DrFilm_filter_yw, film.filter.yWidth);
      // ImageFilm._filterTable is private: the same 16 x 16 table from the same formula (image_film.dart:74-82)
      const int FILTER_TABLE_SIZE = 16;
      int fi = 0;
      for (int y = 0; y < FILTER_TABLE_SIZE; ++y) {
        double fy = (y + 0.5) * film.filter.yWidth / FILTER_TABLE_SIZE;
        for (int x = 0; x < FILTER_TABLE_SIZE; ++x) {
          double fx = (x + 0.5) * film.filter.xWidth / FILTER_TABLE_SIZE;
          rd.f32(fo + OFF_DrFilm_filter_table + 4 * (fi++), film.filter.evaluate(fx, fy));
        }
      }
      if (surfaceIntegrator is PathIntegrator) {
        PathIntegrator pi = surfaceIntegrator;
        rd.i32(OFF_DrRenderDesc_integrator, DR_INTEGRATOR_PATH);
        rd.i32(OFF_DrRenderDesc_max_depth, pi.maxDepth);
      } else if (surfaceIntegrator is DirectLightingIntegrator) {
        DirectLightingIntegrator di = surfaceIntegrator;
        rd.i32(OFF_DrRenderDesc_integrator,
               di.strategy == DirectLightingIntegrator.SAMPLE_ONE_UNIFORM ? DR_INTEGRATOR_DIRECT_ONE : DR_INTEGRATOR_DIRECT_ALL);
        rd.i32(OFF_DrRenderDesc_max_depth, di.maxDepth);
      } else if ('${surfaceIntegrator.runtimeType}' == 'WhittedIntegrator') {  // (told by its name, like the samplers below)
        final dynamic wi = surfaceIntegrator;
        rd.i32(OFF_DrRenderDesc_integrator, DR_INTEGRATOR_WHITTED);
        rd.i32(OFF_DrRenderDesc_max_depth, wi.maxDepth);
      } else if ('${surfaceIntegrator.runtimeType}' == 'AmbientOcclusionIntegrator') {
        // nSamples (already RoundUpPow2'd by the constructor), minDist, maxDist: ambient_occlusion_integrator.dart:62-64; max_depth is not read
        final dynamic ao = surfaceIntegrator;
        rd.i32(OFF_DrRenderDesc_integrator, DR_INTEGRATOR_AO);
        rd.i32(OFF_DrRenderDesc_max_depth, 1);
        final double minDist = ao.minDist;
        final double maxDist = ao.maxDist;
        rd.i32(OFF_DrRenderDesc_ao_nsamples, ao.nSamples);
        rd.f64(OFF_DrRenderDesc_ao_mindist, minDist);
        rd.f64(OFF_DrRenderDesc_ao_maxdist, maxDist);
      } else if ('${surfaceIntegrator.runtimeType}' == 'DiffusePRTIntegrator') {
        // nSamples (already RoundUpPow2'd by the constructor) and lmax: diffuse_prt_integrator.dart:89-90; max_depth is not read
        final dynamic prt = surfaceIntegrator;
        final int lmax = prt.lmax;
        rd.i32(OFF_DrRenderDesc_integrator, DR_INTEGRATOR_DIFFUSE_PRT);
        rd.i32(OFF_DrRenderDesc_max_depth, 1);
        rd.i32(OFF_DrRenderDesc_prt_nsamples, prt.nSamples);
        rd.i32(OFF_DrRenderDesc_prt_lmax, lmax);
      } else if ('${surfaceIntegrator.runtimeType}' == 'GlossyPRTIntegrator') {
        // nSamples (already RoundUpPow2'd by the constructor) and lmax (1 .. 4 on the device): glossy_prt_integrator.dart:130-131; Kd, Ks and
        // roughness (:127-129) are set on the scene, where the BSDF matrix is cached per parameter set; max_depth is not read
        final dynamic gprt = surfaceIntegrator;
        final int lmax = gprt.lmax;
        rd.i32(OFF_DrRenderDesc_integrator, DR_INTEGRATOR_GLOSSY_PRT);
        rd.i32(OFF_DrRenderDesc_max_depth, 1);
        rd.i32(OFF_DrRenderDesc_prt_nsamples, gprt.nSamples);
        rd.i32(OFF_DrRenderDesc_prt_lmax, lmax);
        final _Blob gp = _Blob(SIZEOF_DrGlossyPrtParams);
        try {
          final RGBColor kd = gprt.Kd.toRGB(), ks = gprt.Ks.toRGB();
          gp.f32s(OFF_DrGlossyPrtParams_Kd, [kd.c[0], kd.c[1], kd.c[2]]);
          gp.f32s(OFF_DrGlossyPrtParams_Ks, [ks.c[0], ks.c[1], ks.c[2]]);
          gp.f64(OFF_DrGlossyPrtParams_roughness, gprt.roughness);
          _check(_setGlossyPrt(handle.value, gp.ptr));
        } finally {
          gp.free();
        }
      } else if (surfaceIntegrator is FeatureIntegrator) {  // max_depth is not read
        final FeatureIntegrator feat = surfaceIntegrator;
        rd.i32(OFF_DrRenderDesc_integrator, DR_INTEGRATOR_FEATURE);
        rd.i32(OFF_DrRenderDesc_max_depth, 0);
        rd.i32(OFF_DrRenderDesc_feature_channel, feat.channel);
      } else if (surfaceIntegrator is MaterialIntegrator) {  // max_depth is not read
        final MaterialIntegrator mat = surfaceIntegrator;
        rd.i32(OFF_DrRenderDesc_integrator, DR_INTEGRATOR_MATERIAL);
        rd.i32(OFF_DrRenderDesc_max_depth, 0);
        rd.i32(OFF_DrRenderDesc_material_channel, mat.channel);
      } else {
        _unsupported('surface integrator ${surfaceIntegrator.runtimeType}');
      }
      // The sampler object decides the mode, and a stratified sampler's own public fields (samplers/stratified_sampler.dart:152-155)
      // are the one source of its strata.  (The class is told by its name: on the VM, where dart:ffi runs, runtimeType prints it.)
      final bool stratified = '${sampler.runtimeType}' == 'StratifiedSampler';
      final bool adaptive = '${sampler.runtimeType}' == 'AdaptiveSampler';
      final bool halton = '${sampler.runtimeType}' == 'HaltonSampler';
      final bool random = '${sampler.runtimeType}' == 'RandomSampler';
      if (!stratified && !adaptive && !halton && !random && sampler is! LowDiscrepancySampler) {
        _unsupported('sampler ${sampler.runtimeType}');
      }
      // The device runs the same LD / stratified sampler with one keyed RNG stream per (pixel, LD block) / pixel / (pixel, sample)
      // instead of the task's single serial Random(taskNum) (sampler_renderer.dart:137): same estimator, different numbers.
      if (stratified) {
        dynamic strat = sampler;
        int xPixelSamples = strat.xPixelSamples;
        int yPixelSamples = strat.yPixelSamples;
        bool jitterSamples = strat.jitterSamples;
        // xPixelSamples * yPixelSamples must be a power of two (the library answers DR_ERR_UNSUPPORTED otherwise)
        rd.i32(OFF_DrRenderDesc_spp, xPixelSamples * yPixelSamples);
        rd.i32(OFF_DrRenderDesc_sampler_mode, jitterSamples ? DR_SAMPLER_STRATIFIED : DR_SAMPLER_STRATIFIED_NOJITTER);
        rd.i32(OFF_DrRenderDesc_strat_xsamples, xPixelSamples);
      } else if (adaptive) {
        // the sampler's own fields after its constructor's swapping / rounding / doubling (samplers/adaptive_sampler.dart:53-83,
        // 213-214): powers of two with 2 <= minSamples < maxSamples.  The decision on the device is the contrast test (:170-183).
        dynamic adapt = sampler;
        int minSamples = adapt.minSamples;
        int maxSamples = adapt.maxSamples;
        rd.i32(OFF_DrRenderDesc_spp, maxSamples);
        rd.i32(OFF_DrRenderDesc_sampler_mode, DR_SAMPLER_ADAPTIVE);
        rd.i32(OFF_DrRenderDesc_strat_xsamples, minSamples);  // (the field doubles as minSamples in this mode)
      } else if (halton) {
        // pixelsamples as given (samplers/halton_sampler.dart:106-113): any positive count, nothing is rounded.  One sequence per task
        // over the task's own window; the library refuses the tile split for this sampler (tileCount > 1: DR_ERR_UNSUPPORTED).
        rd.i32(OFF_DrRenderDesc_spp, sampler.samplesPerPixel);
        rd.i32(OFF_DrRenderDesc_sampler_mode, DR_SAMPLER_HALTON);
      } else if (random) {
        // pixelsamples as given (samplers/random_sampler.dart:94-101): it must be a power of two (the library answers DR_ERR_UNSUPPORTED
        // otherwise, so the default of 10 has to be given as 8 or 16)
        rd.i32(OFF_DrRenderDesc_spp, sampler.samplesPerPixel);
        rd.i32(OFF_DrRenderDesc_sampler_mode, DR_SAMPLER_RANDOM);
      } else {
        rd.i32(OFF_DrRenderDesc_spp, sampler.samplesPerPixel);
        rd.i32(OFF_DrRenderDesc_sampler_mode, DR_SAMPLER_COUNTER);
      }
      rd.i64(OFF_DrRenderDesc_seed, seed);
      rd.i32(OFF_DrRenderDesc_task_num, taskNum);         // GetSubWindow rectangle (common.dart:52-73)
      rd.i32(OFF_DrRenderDesc_task_count, taskCount);
      rd.i32(OFF_DrRenderDesc_tile_rank, tileRank);       // this process's share of the 32 x 32 tiles (round-robin)
      rd.i32(OFF_DrRenderDesc_tile_count, tileCount);
      rd.i32(OFF_DrRenderDesc_tile_size, 32);

      // ---- Renderer.render ----
      final int npix = film.width * film.height;
      lxyzw = calloc<Float>(4 * npix);
      rgb = calloc<Float>(3 * npix);
      if (_guideChannels != null && tileCount > 1) {
        _unsupported('renderWithGuides with tileCount > 1 (a sharded guide film)');
      }
      if (tileCount > 1) {
        // one rank of a multi-GPU render: its tiles, ONE ncclReduce(sum) of the full-frame film onto rank 0, which
        // resolves it (dr_render_sharded; commInit has been called by the process).  Ranks > 0 complete with null,
        // like a RenderTask whose output the manager does not merge (render_manager.dart:108-125).
        _check(_renderSharded(handle.value, rd.ptr, 0, lxyzw, rgb));
        if (_commRank() > 0) {
          completer.complete(null);
          return completer.future;
        }
      } else if (_guideChannels != null) {
        final int nch = _guideChannels.length;
        _Blob gd = new _Blob(SIZEOF_DrGuidesDesc);
        blobs.add(gd);
        gd.i32(OFF_DrGuidesDesc_count, nch);
        for (int i = 0; i < nch && i < DR_GUIDES_MAX; ++i) {
          gd.i32(OFF_DrGuidesDesc_channels + 4 * i, _guideChannels[i]);
        }
        _check(renderGuidesCheck(rd.ptr, gd.ptr, nprims));  // (the refusals by name, before anything is allocated)
        // one block of native memory per channel: its film, then its resolved image
        _Blob guideFilms = new _Blob(8 * nch);
        _Blob guideRgbs = new _Blob(8 * nch);
        blobs.add(guideFilms);
        blobs.add(guideRgbs);
        List<_Blob> images = [];
        for (int i = 0; i < nch; ++i) {
          _Blob film4 = new _Blob(16 * npix);
          _Blob rgb3 = new _Blob(12 * npix);
          blobs.add(film4);
          blobs.add(rgb3);
          images.add(rgb3);
          guideFilms.addr(8 * i, film4);
          guideRgbs.addr(8 * i, rgb3);
        }
        _check(_renderGuides(handle.value, rd.ptr, gd.ptr, lxyzw, rgb, guideFilms.ptr, guideRgbs.ptr));
        lastGuides = [];
        for (_Blob image in images) {
          Uint8List bytes = image.ptr.asTypedList(12 * npix);
          lastGuides.add(new Float32List.fromList(bytes.buffer.asFloat32List(bytes.offsetInBytes, 3 * npix)));
        }
      } else {
        _check(_render(handle.value, rd.ptr, lxyzw, rgb));
      }
      _readPilotPicks(handle.value);
      _readSupersampled(handle.value);
      OutputImage out = new OutputImage(film.left, film.top, film.width, film.height,
                                        film.xResolution, film.yResolution,
                                        new Float32List.fromList(rgb.asTypedList(3 * npix)));
      completer.complete(out);
    } catch (e) {
      completer.completeError(e);
    } finally {
      if (handle.value != nullptr) {
        _destroy(handle.value);
      }
      calloc.free(handle);
      if (lxyzw != nullptr) {
        calloc.free(lxyzw);
      }
      if (rgb != nullptr) {
        calloc.free(rgb);
      }
      for (_Blob b in blobs) {
        b.free();
      }
    }
    return completer.future;
  }

  // Per-ray seams are far too fine grained for FFI (one call per ray); like AggregateTestRenderer
  // (aggregate_test_renderer.dart:120-128) they are not part of this renderer.
  Spectrum Li(Scene scene, RayDifferential ray, Sample sample, RNG rng,
              [Intersection isect, Spectrum T]) => new Spectrum(0.0);

  Spectrum transmittance(Scene scene, RayDifferential ray, Sample sample, RNG rng) =>
      new Spectrum(1.0);

  int taskNum;
  int taskCount;
  int device;
  int seed;
  int tileRank;
  int tileCount;
  Sampler sampler;
  Camera camera;
  SurfaceIntegrator surfaceIntegrator;
  VolumeIntegrator volumeIntegrator;
}
