// dr_plan.hip -- the render planner: what a dr_render_device call (or a sample dump) asks for, checked, as a RenderPlan (dr_host.h).
// planRender, in units: the sampler, the integrator's general rules, the camera and the film, the integrator's own rules and its stages, the
// pixel source; planBatches: the sample form and how many camera samples are in flight at once; secondPass: the adaptive sampler's second plan.
// Pure host code: nothing here launches a kernel.  prepareRender (dr_api.hip) allocates what a plan needs.
//
// Host logic restated from the reference where it decides WHAT is traced:
//   sampler window       ImageFilm.getSampleExtent (film/image_film.dart:247-252),
//                        GetSubWindow (core/common.dart:52-73), dartray.dart:1009-1023
//   pixel order          LinearPixelSampler (pixel_samplers/linear_pixel_sampler.dart:29-40)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dr_host.h"

using namespace dr_host;

namespace {

// GetSubWindow (core/common.dart:52-73)
void getSubWindow(int w, int h, int num, int count, int ext[4]) {
  int nx = count, ny = 1;
  while ((nx & 0x1) == 0 && 2 * w * ny < h * nx) {
    nx >>= 1;
    ny <<= 1;
  }
  int xo = num % nx, yo = num / nx;
  double tx0 = (double)xo / nx, tx1 = (double)(xo + 1) / nx;
  double ty0 = (double)yo / ny, ty1 = (double)(yo + 1) / ny;
  auto lerp = [](double t, double v1, double v2) { return v1 * (1.0 - t) + v2 * t; };
  ext[0] = (int)std::floor(lerp(tx0, 0, w));
  ext[1] = std::min((int)std::floor(lerp(tx1, 0, w)), w);
  ext[2] = (int)std::floor(lerp(ty0, 0, h));
  ext[3] = std::min((int)std::floor(lerp(ty1, 0, h)), h);
}

bool knownSamplerMode(const DrRenderDesc* rd) { return rd->sampler_mode >= 0 && rd->sampler_mode <= DR_SAMPLER_RANDOM; }

// ---- unit 1: the sampler mode: its kind, its own rules, the samples per pixel of this plan ----
int planSampler(RenderPlan& P) {
  const DrRenderDesc* rd = P.rd;
  static const SamplerKind kinds[] = {SamplerKind::HostBuffer, SamplerKind::LowDiscrepancy, SamplerKind::Stratified, SamplerKind::Stratified, SamplerKind::Adaptive, SamplerKind::Halton, SamplerKind::Random};
  static_assert(DR_SAMPLER_HOST_BUFFER == 0 && DR_SAMPLER_COUNTER == 1 && DR_SAMPLER_STRATIFIED == 2 && DR_SAMPLER_STRATIFIED_NOJITTER == 3 && DR_SAMPLER_ADAPTIVE == 4 && DR_SAMPLER_HALTON == 5 && DR_SAMPLER_RANDOM == 6, "kinds[] is indexed by sampler_mode");
  P.sampler = knownSamplerMode(rd) ? kinds[rd->sampler_mode] : SamplerKind::LowDiscrepancy;  // (an unknown mode is refused where the pixel source is chosen, as ever)
  P.traits = &kSamplerTraits[(int)P.sampler];
  P.spp = rd->spp;
  switch (P.sampler) {  // (no default: -Wall names a kind this forgets)
    case SamplerKind::HostBuffer: case SamplerKind::LowDiscrepancy: break;
    case SamplerKind::Stratified:  // StratifiedSampler (stratified_sampler.dart:39-54): xs * ys samples per pixel; refused under its own name
      if (P.spp <= 0 || (P.spp & (P.spp - 1)) != 0 || P.spp > 4096)
        return fail(DR_ERR_UNSUPPORTED, "stratified sampler: xsamples * ysamples must be a power of two, at most 4096 (the slot -> pixel maps of the batches are shifts)");
      break;
    case SamplerKind::Adaptive: {
      // AdaptiveSampler (adaptive_sampler.dart:53-83) after its own normalisation, which the host does: maxSamples in spp, minSamples in
      // strat_xsamples.  Powers of two: both passes are LDPixelSample, and the slot -> pixel maps of the batches are shifts.
      const int mn = rd->strat_xsamples, mx = rd->spp;
      if (mn < 2 || mx > 4096 || mn >= mx || (mn & (mn - 1)) != 0 || (mx & (mx - 1)) != 0)
        return fail(DR_ERR_INVALID, "adaptive sampler: minSamples (strat_xsamples) and maxSamples (spp) must be powers of two with 2 <= minSamples < maxSamples <= 4096");
      P.adaptive.pass = 1;
      P.spp = P.adaptive.min = mn;  // (this plan is the first pass)
      P.adaptive.max = mx;
      break;
    }
    case SamplerKind::Halton:
      // HaltonSampler (halton_sampler.dart:31-48): any positive pixelsamples; ONE sequence per task over the task's own window, so the
      // tile round-robin -- a share of the pixels -- has nothing to deal out
      if (rd->spp < 1) return fail(DR_ERR_INVALID, "halton sampler: pixelsamples (spp) must be at least 1");
      if (rd->tile_count > 1) return fail(DR_ERR_UNSUPPORTED, "halton sampler: tile_count > 1 (the tile round-robin deals out pixels; a task's Halton sequence is not bound to pixels: split by task_num / task_count)");
      P.spp = 1;  // (one slot per accepted sample)
      break;
    case SamplerKind::Random:  // RandomSampler (random_sampler.dart:94-101): pixelsamples as given -- nothing rounds it, so the limit is refused under its own name
      if (P.spp <= 0 || (P.spp & (P.spp - 1)) != 0 || P.spp > 4096)
        return fail(DR_ERR_UNSUPPORTED, "random sampler: pixelsamples (spp) must be a power of two, at most 4096 (the slot -> pixel maps of the batches are shifts)");
      break;
  }
  const int spp = P.spp;
  if (P.traits->pow2Spp && (spp <= 0 || (spp & (spp - 1)) != 0)) return fail(DR_ERR_INVALID, "spp must be a power of two (low_discrepancy_sampler.dart:43-49)");
  if (spp > 4096) return fail(DR_ERR_UNSUPPORTED, "spp > 4096 (one pixel's shuffle table of a 16-pixel sampler group would not fit the LDS)");
  return DR_OK;
}

// ---- unit 2: the integrator's kind and the rules every kind shares; what follows from the kind and the scene alone: dlSpec, envStage, the state layout ----
int planIntegrator(RenderPlan& P) {
  DrScene* sc = P.sc;
  const DrRenderDesc* rd = P.rd;
  if (!knownIntegrator(rd->integrator)) return fail(DR_ERR_INVALID, "unknown integrator");
  P.integrator = (IntegratorKind)rd->integrator;  // (the kinds are the ABI's values: IntegratorKind)
  P.integ = &kIntegratorTraits[rd->integrator];
  if (P.integ->depthBelowOne && rd->max_depth < 1) return fail(DR_ERR_INVALID, P.integ->depthBelowOne);
  if (rd->max_depth < 0 || rd->max_depth > 64) return fail(DR_ERR_INVALID, "max_depth out of range");
  if (P.integ->adaptive && P.sampler == SamplerKind::Adaptive) return fail(DR_ERR_UNSUPPORTED, P.integ->adaptive);
  // DirectLighting over mirror / glass recurses through SpecularReflect / SpecularTransmit (integrator.dart:187-290):
  // an explicit per-slot stack and one round of the stage loop per vertex of the ray tree (k_shade_spec); so does Whitted
  P.dlSpec = P.integ->specularRounds && sc->hasSpecular;
  // k_env (dr_kernels.hip): the environment-map work of a plain-triangle scene's path stages runs in its own kernel
  P.envStage = P.integ->pathStages && sc->d.hasEnv && !(sc->d.nquads || sc->d.hasSpec || sc->d.srec);
  // State layout (see LayoutOps): the four-slot sub-tiles for the renders whose lists thin out early.  Which one is MEASURED on
  // the render's own work: the first calibration batch -- rendered into the film like any other -- runs in the 64-slot layout
  // and its stage lists say how fast the paths die; when less than half of the slots are still alive at the second bounce the
  // rest of the render, and every later render of the scene, uses the four-slot sub-tiles (C5: 0.38 -> sp4; C2 0.80, C4: 64-slot).
  // DARTRAY_STATE_LAYOUT=64|4 forces one, dr_scene_set_state_layout stores one; renders too small for a pilot keep round 3's
  // rule (plain-triangle scenes under an environment map: sp4).
  const DrOpt layoutEnv = dr_opt("DARTRAY_STATE_LAYOUT");
  P.layoutKnown = layoutEnv || sc->stateLayout != 0 || !P.integ->pathStages || !P.traits->pixelBound;  // (not pixel bound: no pilot)
  const bool sparseLayout = layoutEnv ? layoutEnv.toInt(0) == 4 : (sc->stateLayout ? sc->stateLayout == 4 : P.envStage);
  P.L = sparseLayout ? &kLayoutSp4 : &kLayout64;
  P.maxStateWords = P.layoutKnown ? P.L->stateWords : std::max(kLayout64.stateWords, kLayoutSp4.stateWords);
  return DR_OK;
}

// ---- unit 3: the camera and the film into rp; the sample slots ----
int planCameraAndFilm(RenderPlan& P) {
  DrScene* sc = P.sc;
  const DrRenderDesc* rd = P.rd;
  RenderParams& rp = P.rp;
  memset(&rp, 0, sizeof(rp));
  memcpy(rp.r2c, rd->camera.raster_to_camera, sizeof(rp.r2c));
  memcpy(rp.c2w, rd->camera.camera_to_world, sizeof(rp.c2w));
  rp.lensRadius = rd->camera.lens_radius;
  rp.focalDistance = rd->camera.focal_distance;
  rp.shutterOpen = rd->camera.shutter_open;
  rp.shutterClose = rd->camera.shutter_close;
  rp.cameraType = rd->camera.type;
  if (rp.cameraType < DR_CAMERA_PERSPECTIVE || rp.cameraType > DR_CAMERA_ENVIRONMENT) return fail(DR_ERR_INVALID, "unknown camera type");
  rp_film(rp, rd->film);
  rp.integrator = rd->integrator;
  rp.maxDepth = rd->max_depth;
  rp.spp = P.spp;
  rp.sppShift = 0;
  while ((1 << rp.sppShift) < P.spp) ++rp.sppShift;
  rp.nLights = (int)sc->d.nlights;
  const SlotCounts slots = integratorSlots(P.integrator, sc, sc->d.nlights);
  rp.nFloats = slots.nFloats();
  rp.n1D = slots.n1D;
  rp.blocks = P.integ->sceneSlots && sc->dlMulti ? sc->dlBlocks.p : nullptr;
  rp.nBlocks = sc->dlNBlocks;
  return DR_OK;
}

// ---- unit 4: the integrator's own rules and its stages: one plan function per integrator that has rules, and the switch that calls them ----

// Only a Lambertian matte: rho2's 36-sample estimate of the other lobes has no device function outside the kernels that own them, so a scene with
// any other material is refused by name (diffuse PRT, use probes)
int matteOnly(const RenderPlan& P, const char* integratorName) {
  static const char* const names[] = {"matte with sigma != 0 (Oren-Nayar)", "matte", "mirror", "glass", "plastic"};
  const std::vector<int32_t>& mats = P.sc->prtMaterials;
  for (size_t i = 0; i < mats.size(); ++i)
    if (mats[i] != DR_MATERIAL_MATTE)
      return fail(DR_ERR_UNSUPPORTED, std::string(integratorName) + ": material " + names[std::min(3, std::max(-1, mats[i])) + 1] + " (material " + std::to_string(i) +
                                          " of the scene) is not supported: only matte with sigma 0 is");
  return DR_OK;
}

// The stages of an integrator that sends its rays in rounds (Rounds, dr_host.h): a round is one stage more than its rays, since the last ray is
// folded in by a stage that queues nothing
void planRounds(RenderPlan& P, int requested) {
  P.rounds = Rounds::of(requested);
  P.nStages = P.rounds.perRound + 1;
}

// AmbientOcclusionIntegrator (ambient_occlusion_integrator.dart:24-26,55-60): nSamples = RoundUpPow2(ns) occlusion rays per camera
// hit, one per stage, in rounds
int planAmbientOcclusion(RenderPlan& P) {
  const DrRenderDesc* rd = P.rd;
  if (rd->ao_nsamples < 1) return fail(DR_ERR_INVALID, "ambient occlusion integrator: nsamples must be at least 1");
  if (rd->ao_nsamples > 4096) return fail(DR_ERR_INVALID, "ambient occlusion integrator: nsamples above 4096 after rounding up to a power of two (the samplers' cap)");
  if (!(rd->ao_mindist >= 0.0)) return fail(DR_ERR_INVALID, "ambient occlusion integrator: mindist must not be negative");
  if (!(rd->ao_maxdist > rd->ao_mindist)) return fail(DR_ERR_INVALID, "ambient occlusion integrator: maxdist must be greater than mindist");
  planRounds(P, rd->ao_nsamples);
  P.ao.minDist = rd->ao_mindist;
  P.ao.maxDist = rd->ao_maxdist;
  return DR_OK;
}

// Feature: the camera hit itself, one stage, nothing traced behind it
int planFeature(RenderPlan& P) {
  int code = DR_OK;
  if (const char* why = featureRefusal(P.rd->feature_channel, P.sc->d.ntris, &code)) return fail(code, why);
  P.feature.channel = P.rd->feature_channel;
  P.nStages = 1;
  return DR_OK;
}

// DiffusePRTIntegrator (diffuse_prt_integrator.dart:24-31,83-87): nSamples = RoundUpPow2(ns) occlusion rays per camera hit, one
// per stage, in ambient occlusion's rounds.  Materials other than a Lambertian matte are refused by name (matteOnly).
int planDiffusePRT(RenderPlan& P) {
  if (const char* why = prtRefusal(P.rd->prt_lmax, P.rd->prt_nsamples, true)) return fail(DR_ERR_INVALID, why);
  if (int rc = matteOnly(P, "diffuse PRT")) return rc;
  planRounds(P, P.rd->prt_nsamples);
  P.prt.lmax = P.rd->prt_lmax;
  return DR_OK;
}

// GlossyPRTIntegrator (glossy_prt_integrator.dart:24-25,118-125): DiffusePRT's rays, stages and rounds -- every ray is traced --
// and no material function is read, so no material is refused
int planGlossyPRT(RenderPlan& P) {
  if (const char* why = gprtRefusal(P.rd->prt_lmax, P.rd->prt_nsamples, true)) return fail(DR_ERR_INVALID, why);
  planRounds(P, P.rd->prt_nsamples);
  P.gprt.lmax = P.rd->prt_lmax;
  P.gprt.words = std::max(1, P.rounds.nSamples / 32);
  return DR_OK;
}

// UseProbesIntegrator (use_probes_integrator.dart:90-162): the camera hit and the scene's probe grid, one stage, nothing traced
// behind it.  Materials other than a Lambertian matte are refused by name, as under diffuse PRT (matteOnly).
int planUseProbes(RenderPlan& P) {
  const DrScene* sc = P.sc;
  if (sc->probes.lmax == 0) return fail(DR_ERR_INVALID, "use probes: no probe grid is set on the scene (dr_scene_set_probes)");
  if (sc->probes.includeDirect == 0)
    return fail(DR_ERR_UNSUPPORTED, "use probes: a grid with includeDirect 0 is not supported (that path adds UniformSampleAllLights at every hit); bake with directlighting true");
  if (int rc = matteOnly(P, "use probes")) return rc;
  P.nStages = 1;
  return DR_OK;
}

// Material: the camera hit's material colour or emitted radiance, one stage, nothing traced behind it
int planMaterial(RenderPlan& P) {
  if (const char* why = materialRefusal(P.rd->material_channel)) return fail(DR_ERR_INVALID, why);
  P.material.channel = P.rd->material_channel;
  P.nStages = 1;
  return DR_OK;
}

// What the stages read of a sample: which LD blocks (genMask), the RNG draws beyond the vector (needTail); the shade launchers' grid
void planSampleReads(RenderPlan& P) {
  DrScene* sc = P.sc;
  const DrRenderDesc* rd = P.rd;
  RenderParams& rp = P.rp;
  rp.dlSpecular = P.dlSpec ? 1 : 0;
  rp.deferredNee = P.integ->pathStages ? 1 : 0;
  rp.genMask = 0ull;
  rp.genSlowDraws = dr_opt("DARTRAY_GEN_SLOW_DRAWS").set ? 1 : 0;
  if (!(P.traits->deviceGenerated && P.traits->floatForm) && P.integ->pathStages && !rp.blocks && !dr_opt("DARTRAY_GEN_ALL_BLOCKS").set) {
    // What the path kernels read of a pixel sample (dr_kernels.hip: k_raygen, load_shade_in, k_film): the image sample,
    // the lens sample of a thin-lens camera, and per SAMPLE_DEPTH level b <= maxDepth the light number, the light
    // sample (component + position), the BSDF and path directions; the two uComponent slots only where a material has
    // more than one lobe.  Never read: the time sample, the volume integrator's two slots, levels beyond maxDepth.
    const bool general = sc->d.nquads || sc->d.hasSpec || sc->d.srec;
    uint64_t m = 1ull | (rd->camera.lens_radius > 0.0 ? 2ull : 0ull);
    for (int b = 0; b < 3 && b <= rd->max_depth; ++b) {
      m |= 3ull << (3 + 4 * b);
      if (general) m |= 12ull << (3 + 4 * b);
      m |= 7ull << (3 + rp.n1D + 3 * b);
    }
    rp.genMask = m;  // (only the LD sampler reads it: a device sampler that writes floats leaves no block out)
  }
  rp.samplerMode = P.sampler == SamplerKind::Adaptive ? DR_SAMPLER_COUNTER : rd->sampler_mode;  // (both adaptive passes are the LD sampler's keyed streams)
  rp.seed = (uint64_t)rd->seed;
  const int perNee = rp.nLights > 0 ? 7 : 0;
  P.needTail = P.integ->pathStages && rd->max_depth >= 3 ? (rd->max_depth - 2) * (perNee + 3) + std::max(0, rd->max_depth - 3) : 0;
  rp.maxTail = rd->max_tail;
  P.sgrid = g_numCU;  // the shade launchers size their grid per CU (DR_SHADE_GRID), grid-stride over the active list
}

// the stages: where a stage's DirectStage entry comes from, and how many stages a round of the stage loop runs
int planStages(RenderPlan& P) {
  DrScene* sc = P.sc;
  RenderParams& rp = P.rp;
  rp.dstages = sc->dlStages.p;
  rp.nDirectStages = 0;
  int rc = DR_OK;
  switch (P.integrator) {  // (no default: -Wall names a kind this forgets)
    case IntegratorKind::DirectAll: rp.nDirectStages = sc->dlNStages; P.nStages = rp.nDirectStages + 1; break;  // the scene's table from its start
    case IntegratorKind::DirectOne:  // strategy "one": the last entry of the scene's stage table, an arithmetic slot layout
      rp.dstages += sc->dlNStages;
      rp.nDirectStages = sc->d.nlights ? 1 : 0;
      P.nStages = rp.nDirectStages + 1;
      break;
    case IntegratorKind::Path: P.nStages = P.rd->max_depth + 2; break;
    case IntegratorKind::Whitted: P.nStages = rp.nLights + 1; break;  // one per light
    case IntegratorKind::AmbientOcclusion: rc = planAmbientOcclusion(P); break;
    case IntegratorKind::Feature: rc = planFeature(P); break;
    case IntegratorKind::DiffusePRT: rc = planDiffusePRT(P); break;
    case IntegratorKind::GlossyPRT: rc = planGlossyPRT(P); break;
    case IntegratorKind::UseProbes: rc = planUseProbes(P); break;
    case IntegratorKind::Material: rc = planMaterial(P); break;
  }
  if (rc) return rc;
  planSampleReads(P);
  return DR_OK;
}

// ---- unit 5: the pixel source: the caller's list, the task's / tile share's pixels, or -- not pixel bound -- a window of the Halton sequence ----

int planHostPixels(RenderPlan& P) {
  const DrRenderDesc* rd = P.rd;
  if (rd->nsamples <= 0 || rd->nsamples % P.spp != 0 || !rd->pixel_xy || !rd->sample_vec)
    return fail(DR_ERR_INVALID, "host-buffer sampler: nsamples must be a positive multiple of spp with pixel_xy and sample_vec set");
  if (rd->sample_stride < P.rp.nFloats) return fail(DR_ERR_INVALID, "sample_stride smaller than the sample vector");
  if (P.needTail > 0 && (!rd->tail || rd->max_tail < P.needTail))
    return fail(DR_ERR_INVALID, "host-buffer sampler: tail buffer missing or max_tail too small for max_depth");
  P.packedTail = P.needTail > 0 && rd->tail_offsets != nullptr;  // (its device buffers are sized per batch: BatchRunner::loadSamples)
  if (P.packedTail && rd->tail_offsets[rd->nsamples] < rd->tail_offsets[0])
    return fail(DR_ERR_INVALID, "host-buffer sampler: tail_offsets must be non-decreasing");
  const int64_t np = rd->nsamples / P.spp;
  P.pixels.resize(np);
  for (int64_t i = 0; i < np; ++i) P.pixels[i] = make_int2(rd->pixel_xy[2 * i], rd->pixel_xy[2 * i + 1]);
  return DR_OK;
}

int planBoundPixels(RenderPlan& P) {
  if (!knownSamplerMode(P.rd)) return fail(DR_ERR_INVALID, "unknown sampler mode");
  enumeratePixels(P.rp, P.rd, P.pixels);
  return DR_OK;
}

// Halton: the task's window as the reference hands it to the sampler (GetSubWindow's extents as they are: see enumeratePixels)
int planHaltonWindow(RenderPlan& P) {
  const DrRenderDesc* rd = P.rd;
  const RenderParams& rp = P.rp;
  int ext[4];
  getSubWindow(rp.extW, rp.extH, rd->task_num, std::max(1, rd->task_count), ext);
  const int w = ext[1] - ext[0], h = ext[3] - ext[2], delta = std::max(w, h);
  P.pixels.clear();
  const int32_t win[5] = {ext[0], ext[2], ext[0] + w - 1, ext[2] + h - 1, delta};
  memcpy(P.halton.win, win, sizeof(win));
  const uint64_t wanted = w > 0 && h > 0 ? (uint64_t)rd->spp * (uint64_t)delta * (uint64_t)delta : 0ull;  // wantedSamples (halton_sampler.dart:35-36)
  if (wanted >= (1ull << 53)) return fail(DR_ERR_UNSUPPORTED, "halton sampler: pixelsamples * max(width, height)^2 must stay below 2^53 (RadicalInverse takes the index through a double)");
  // (the key pixel of index k is (extX0 + k % extW, extY0 + k / extW): k_gen_halton)
  if (wanted / (uint64_t)std::max(1, rp.extW) >= (uint64_t)(0x7fffffff - std::abs(rp.extY0)))
    return fail(DR_ERR_UNSUPPORTED, "halton sampler: pixelsamples * max(width, height)^2 must stay below 2^31 rows of the sampler extent (the in-Li streams are keyed by the index as a pixel of the extent)");
  P.npixTotal = (size_t)wanted;
  // film_samples, as for the other modes: the window's pixels that the film holds x pixelsamples (what the sequence aims at)
  const int64_t fw = std::min(ext[1], rp.left + rp.width) - std::max(ext[0], rp.left), fh = std::min(ext[3], rp.top + rp.height) - std::max(ext[2], rp.top);
  P.filmSamples = fw > 0 && fh > 0 ? (uint64_t)fw * (uint64_t)fh * (uint64_t)rd->spp : 0ull;
  return DR_OK;
}

// The mode's rules that have always run behind the integrator's, max_depth's and the camera's refusals (strat_xsamples reads only spp, but a descriptor
// that also names an unknown integrator keeps that refusal); then which pixels
int planPixelSource(RenderPlan& P) {
  DrScene* sc = P.sc;
  const DrRenderDesc* rd = P.rd;
  const RenderParams& rp = P.rp;
  if (P.sampler == SamplerKind::Stratified) {
    P.strat.x = rd->strat_xsamples;
    if (P.strat.x <= 0 || P.spp % P.strat.x != 0)
      return fail(DR_ERR_INVALID, "stratified sampler: strat_xsamples must be positive and divide spp (spp = xsamples * ysamples)");
  }
  // roundSize is the identity (stratified_sampler.dart:63-65, halton_sampler.dart:102-104, random_sampler.dart:90-92) while the scene's DirectLighting slot layout is
  // LowDiscrepancySampler's rounded one, so a light's nsamples must be its own rounding
  if (P.traits->identityRoundSize && P.integ->sceneSlots)
    for (int n : sc->lightNSamples)
      if (n > 1 && (n & (n - 1)) != 0) return fail(DR_ERR_UNSUPPORTED, P.traits->identityRoundSize);
  if (P.sampler == SamplerKind::Adaptive && rp.blocks && P.adaptive.max > 1024)
    return fail(DR_ERR_UNSUPPORTED, "adaptive sampler: maxSamples > 1024 with LD blocks of several entries per sample (DirectLighting with nsamples > 1): the float-form sampler's table exceeds the LDS");
  const int rc = P.sampler == SamplerKind::HostBuffer ? planHostPixels(P) : P.traits->pixelBound ? planBoundPixels(P) : planHaltonWindow(P);
  if (rc) return rc;
  if (P.traits->pixelBound) {
    P.npixTotal = P.pixels.size();
    P.filmSamples = 0;
    for (const int2& p : P.pixels)
      if (p.x >= rp.left && p.x < rp.left + rp.width && p.y >= rp.top && p.y < rp.top + rp.height) P.filmSamples += P.spp;
  }
  if (P.nStages > CounterLayout::maxStages()) return fail(DR_ERR_UNSUPPORTED, "too many stages");
  return DR_OK;
}

}  // namespace

namespace dr_host {

void rp_film(RenderParams& rp, const DrFilm& f) {
  rp.xres = f.xres;
  rp.yres = f.yres;
  // image_film.dart:61-65
  rp.left = (int)std::ceil(f.xres * (double)f.crop[0]);
  rp.width = std::max(1, (int)std::ceil(f.xres * (double)f.crop[1]) - rp.left);
  rp.top = (int)std::ceil(f.yres * (double)f.crop[2]);
  rp.height = std::max(1, (int)std::ceil(f.yres * (double)f.crop[3]) - rp.top);
  rp.fxw = f.filter_xw;
  rp.fyw = f.filter_yw;
  rp.invX = 1.0 / (double)f.filter_xw;  // filter.dart:33-37
  rp.invY = 1.0 / (double)f.filter_yw;
  // ImageFilm.getSampleExtent (image_film.dart:247-252)
  int e0 = (int)std::floor(rp.left + 0.5 - rp.fxw);
  int e1 = (int)std::ceil(rp.left + 0.5 + rp.width + rp.fxw);
  int e2 = (int)std::floor(rp.top + 0.5 - rp.fyw);
  int e3 = (int)std::ceil(rp.top + 0.5 + rp.height + rp.fyw);
  rp.extX0 = e0;
  rp.extY0 = e2;
  rp.extW = e1 - e0;
  rp.extH = e3 - e2;
}

// Raster pixels one call traces in counter mode, in trace order.  task_*: the reference's
// GetSubWindow rectangle; tile_*: tile_size^2 tiles dealt round-robin over ranks.  The dead
// border row/column of the sampler window (W+1 x H+1 for the box filter, image_film.dart:247-252)
// is traced as the reference does; a border sample only reaches the film when imageX/Y is integral.
void enumeratePixels(const RenderParams& rp, const DrRenderDesc* rd, std::vector<int2>& pixels) {
  // NB the reference hands GetSubWindow's extents to the sampler as they are (dartray.dart:1009-1022): they are
  // computed from 0 and ignore the sample extent's origin (common.dart:69-72), so a cropped film -- or a filter
  // wider than half a pixel, whose extent starts at -1 -- samples the window [0, w) x [0, h) instead of
  // [x0, x0 + w) x [y0, y0 + h).  Reproduced: the window is an input of the path.
  int ext[4];
  getSubWindow(rp.extW, rp.extH, rd->task_num, std::max(1, rd->task_count), ext);
  const int ts = rd->tile_size > 0 ? rd->tile_size : 32;
  const int ntx = (rp.extW + ts - 1) / ts;
  const bool tiled = rd->tile_count > 1;
  pixels.clear();
  pixels.reserve((size_t)(ext[1] - ext[0]) * (ext[3] - ext[2]) / (tiled ? rd->tile_count : 1) + 1024);
  if (!tiled) {  // LinearPixelSampler order (linear_pixel_sampler.dart:29-40)
    for (int y = ext[2]; y < ext[3]; ++y)
      for (int x = ext[0]; x < ext[1]; ++x) pixels.push_back(make_int2(x, y));
  } else {  // tile-major so that a batch covers whole tiles (coherent camera rays)
    const int nty = (rp.extH + ts - 1) / ts;
    for (int ty = 0; ty < nty; ++ty)
      for (int tx = 0; tx < ntx; ++tx) {
        if ((ty * ntx + tx) % rd->tile_count != rd->tile_rank) continue;
        for (int y = std::max(ty * ts, ext[2]); y < std::min((ty + 1) * ts, ext[3]); ++y)
          for (int x = std::max(tx * ts, ext[0]); x < std::min((tx + 1) * ts, ext[1]); ++x)
            pixels.push_back(make_int2(x, y));
      }
  }
}

// What the call asks for, checked, as RenderParams + the facts every later unit reads; which pixels it traces.  Callable without a film (the two
// sample dumps plan this way).  The units run in the order their checks always ran in, so that of two broken rules the same one wins
// (tests/test_gpu_integrator_plan.py holds a pair per seam).
int planRender(RenderPlan& P) {
  int rc = planSampler(P);
  if (!rc) rc = planIntegrator(P);
  if (!rc) rc = planCameraAndFilm(P);
  if (!rc) rc = planStages(P);
  if (!rc) rc = planPixelSource(P);
  return rc;
}

// The sample form and the batches: how many camera samples are in flight at once.
int planBatches(RenderPlan& P) {
  DrScene* sc = P.sc;
  const DrRenderDesc* rd = P.rd;
  const RenderParams& rp = P.rp;
  const int spp = P.spp;
  // Sample vectors: the on-device LD sampler stores permuted indices + scrambles (compact form) whenever every LD block
  // has one entry per pixel sample; host buffers and multi-entry blocks (DirectLighting with nsamples > 1) use floats.
  SampleForm& sf = P.sf;
  sf.compact = !P.traits->floatForm && rp.blocks == nullptr;  // (the stratified, Halton and random samplers' values are no function of an LD index: floats)
  if (!P.traits->floatForm && !sf.compact && spp > 1024)  // (the LD sampler writing floats)
    return fail(DR_ERR_UNSUPPORTED, "spp > 1024 with LD blocks of several entries per sample (DirectLighting with nsamples > 1): the float-form sampler's table exceeds the LDS");
  sf.nFloats = rp.nFloats;
  // (not sampler_block_count(rp) of dr_sampler_lhs.h, which answers rp.nBlocks under rp.blocks: this counts the field layout's slots whatever rp.blocks says)
  sf.nBlocks = 3 + rp.n1D + (rp.nFloats - 5 - rp.n1D) / 2;
  sf.idxShift = spp > 256 ? 1 : 0;
  // what the workspace's sample region is sized for: this form; adaptive: the second pass's (same blocks, wider indices above 256 spp)
  P.wsSf = sf;
  if (P.sampler == SamplerKind::Adaptive) P.wsSf.idxShift = P.adaptive.max > 256 ? 1 : 0;
  // Camera samples in flight per batch.  The throughput end is one batch per image (2^28 slots: C2's whole sampler window, 64 GB of a
  // 288 GB MI355X); a scene's FIRST big render -- all a one-shot host ever does (Renderer.render once per task, dartray.dart:574) --
  // stays at 2^27 (C2: three batches, 21 GB, whose hipMalloc does not wait for the driver to scrub 64 GB: profiles/r05_alloc_probe.txt)
  // and the workspace grows to the image when the same scene is rendered again (a frame loop, bench.py's steps: + 3 % steady state).
  const DrOpt bitsOpt = dr_opt("DARTRAY_BATCH_BITS");
  const int slotBits = std::min(28, std::max(16, bitsOpt ? bitsOpt.toInt(28) : (sc->bigRenders == 0 ? 27 : 28)));
  uint64_t maxSlots = 1ull << slotBits;
  {
    // path state per camera sample: 164 B of ray / hit / NEE state, 20 B of queues and the sample vector (24 B of permuted
    // indices in the compact form, 4 B per float otherwise; + the RNG tail in host-buffer mode) and the integrator's side buffers.  On a
    // device with less free memory the batch shrinks instead of failing (results do not depend on the batch size).
    const uint64_t tailPerSlot = !(!P.traits->deviceGenerated && P.needTail > 0) ? 0ull
                                 : (P.packedTail ? 16ull + 8ull * ((rd->tail_offsets[rd->nsamples] - rd->tail_offsets[0]) / (uint64_t)rd->nsamples + 1ull)
                                                 : (uint64_t)rd->max_tail * 8);
    const uint64_t perSlot = (uint64_t)P.maxStateWords * 4 + (uint64_t)(P.wsSf.svWords() + 15) / 16 + 20 + tailPerSlot + (!P.traits->deviceGenerated ? (uint64_t)rd->sample_stride * 4 : 0) +
                             (sf.compact ? (uint64_t)(16 * sf.nBlocks + spp - 1) / spp : 0) +  // scramble words + generator states, per (block, pixel)
                             sideBufferBytesPerSlot(P);
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
      const uint64_t have = (uint64_t)sc->ws.cap * ((uint64_t)sc->ws.stateWords * 4 + sc->ws.svWords / 16 + 20);
      const uint64_t budget = (uint64_t)(0.9 * (double)freeB) + have;
      // (+ 1/4: the slack that lets a slightly larger window still go as one batch, below)
      while (maxSlots > (1ull << 16) && std::min<uint64_t>(maxSlots + maxSlots / 4, (uint64_t)P.npixTotal * spp) * perSlot > budget) maxSlots >>= 1;
    }
  }
  // Equal batches, and no tiny tail batch: every stage launch costs ~0.4 ms of ramp-up and tail however small it is
  // (the sampler window of a 1024 x 1024 film is 1025 x 1025 pixels -- 2^20 + 2049).
  const uint64_t pixCapBatch = std::max<uint64_t>(1, maxSlots / spp);
  P.nBatches = (P.npixTotal + pixCapBatch - 1) / pixCapBatch;
  if (P.traits->pixelBound && P.nBatches > 1 && P.npixTotal <= pixCapBatch + pixCapBatch / 4) P.nBatches = 1;  // (else: a batch's range is its slot capacity at most)
  P.pixPerBatch = (uint32_t)((P.npixTotal + P.nBatches - 1) / P.nBatches);
  P.cap = P.pixPerBatch * (uint32_t)spp;
  P.wsCap = P.cap;
  P.wsPix = P.pixPerBatch;
  if (P.sampler == SamplerKind::Adaptive) {
    // The second pass runs in the workspace of the first: how many pixels are flagged is only known once the first pass has run, and
    // a workspace sized for the worst case (every pixel at maxSamples) would be max / min times the first pass's.  Its batches hold
    // as many slots as a first-pass batch -- or 2^22 where those are smaller, so that a small image's flagged pixels still go as a
    // few launches -- and never more than every pixel of the render at maxSamples, nor less than one pixel.
    const uint64_t worst = (uint64_t)P.npixTotal * (uint64_t)P.adaptive.max;
    const uint64_t slots2 = std::max<uint64_t>((uint64_t)P.adaptive.max, std::min<uint64_t>(worst, std::max<uint64_t>(P.cap, std::min<uint64_t>(1ull << 22, maxSlots))));
    P.adaptive.pixCap = (uint32_t)(slots2 / (uint64_t)P.adaptive.max);
    P.wsCap = std::max(P.cap, P.adaptive.pixCap * (uint32_t)P.adaptive.max);
    P.wsPix = std::max(P.pixPerBatch, P.adaptive.pixCap);
  }
  return DR_OK;
}

// The second pass of an adaptive render: the nFlagged pixels of the device list at maxSamples, as ordinary counter-mode batches.
// Everything that depends on the sample count is derived again; no pilot runs (the first pass's choices stand).
RenderPlan secondPass(const RenderPlan& P, uint32_t nFlagged) {
  RenderPlan Q = P;
  Q.adaptive.pass = 2;
  Q.spp = Q.rp.spp = P.adaptive.max;
  Q.rp.sppShift = 0;
  while ((1 << Q.rp.sppShift) < Q.spp) ++Q.rp.sppShift;
  Q.sf = P.wsSf;
  Q.lazyGen = lazyGenFor(Q);
  Q.calibrateTrace = Q.measureLayout = false;
  Q.npixTotal = nFlagged;
  Q.nBatches = ((uint64_t)nFlagged + P.adaptive.pixCap - 1) / P.adaptive.pixCap;
  Q.pixPerBatch = (uint32_t)(((uint64_t)nFlagged + Q.nBatches - 1) / Q.nBatches);
  Q.cap = Q.pixPerBatch * (uint32_t)Q.spp;
  return Q;
}

bool lazyGenFor(const RenderPlan& P) {
  return P.sf.compact && P.rp.genMask != 0ull && P.integ->pathStages && P.coherentCamera && !P.sc->d.nquads && P.spp >= 64 &&
         !dr_opt("DARTRAY_LAZY_GEN").isZero();
}

}  // namespace dr_host
