// dr_host.h -- what the host units of the library share (internal; not part of the C ABI):
//   dr_api.hip          options, prepareRender (what a RenderPlan needs on the device), the entry points
//   dr_plan.hip         the render planner (RenderPlan: planRender in units, planBatches, secondPass)
//   dr_scene_build.hip  dr_scene_create / dr_scene_destroy (SceneBuilder)
//   dr_batch.hip        one batch through the stage loop (BatchRunner), the batch loop, the pilot
// Whatever has external linkage here lives in namespace dr_host (each unit says `using namespace dr_host;`); what a single unit uses
// stays in that unit's anonymous namespace.
#ifndef DR_HOST_H
#define DR_HOST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "dr_kernels.h"
#include "dr_prt.h"
#include "dr_gprt.h"
#include "dr_probes.h"

namespace dr_host {

extern int g_device;  // dr_init's device (-1 before it)
extern int g_numCU;   // its compute units (256 before it)

int fail(int code, const std::string& msg);  // dr_api.hip: sets dr_last_error(), returns code
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(DR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t count) {
    if (count <= n && p) return hipSuccess;
    release();
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  size_t bytes() const { return p ? std::max<size_t>(n, 1) * sizeof(T) : 0; }
  ~DevBuf() { release(); }
};

struct Workspace {
  uint32_t cap = 0;
  int stateWords = 0;  // words per slot the tiles were sized for
  int svWords = 0, maxTail = 0;  // svWords: 4-byte words of the sample region of one tile
  uint32_t pixCap = 0;
  DevBuf<float> tiles;  // the tiled path state (see BatchState in dr_kernels.h): cap/64 tiles of 64*41+svWords words
  DevBuf<uint32_t> scr;  // compact samples: scramble words [2 * nBlocks][pixCap]
  DevBuf<uint2> genState;  //   and the streams' generator states behind their burn-in draws [nBlocks][pixCap] (k_gen_burnin)
  DevBuf<double> tail;
  DevBuf<unsigned long long> tailOff;  // packed tail (DrRenderDesc.tail_offsets): the batch's nslots + 1 offsets
  DevBuf<uint32_t> activeA, activeB, closestQ, anyQ, counters, spill;
  DevBuf<uint32_t> envQ;  // plain-triangle scenes under an environment map: k_env's list of a stage (cap entries)
  DevBuf<uint8_t> alive;  // lazy sample generation: [3][groups of 64 batch pixels] = a path of the group is alive at bounce 0 / 1 / 2
  size_t spillHalf = 0;
  DevBuf<uint32_t> roundA, roundB;  // DirectLighting over mirror / glass: the slots whose child ray is traced next round; ambient occlusion: the slots that hit
  DevBuf<float> specFrames;         //   [maxDepth][cap] SpecFrame
  DevBuf<int32_t> specSp;           //   [cap]
  DevBuf<int2> pix;
  DevBuf<int2> adaptList;       // DR_SAMPLER_ADAPTIVE: the raster pixels the first pass flagged (k_adaptive_decide), the second pass's pixel array
  DevBuf<uint32_t> adaptCount;  //   [0] their number, [1] those inside the film window
  struct Halton {  // DR_SAMPLER_HALTON, sized for a batch (beside `pix`, where k_gen_halton writes the slots' anchor pixels)
    DevBuf<unsigned long long> idx;  // the sequence index of every slot of the batch,
    DevBuf<int2> keyPix;             //   the pixel whose index in the sampler extent is that index: the shade stages' pixel array (k_gen_halton)
    DevBuf<uint32_t> blk;            //   the selection's per-workgroup counts / offsets; the word behind them: the batch's slot count
    hipError_t alloc(uint32_t cap) {
      hipError_t e = idx.alloc(cap);
      if (e == hipSuccess) e = keyPix.alloc(cap);
      return e != hipSuccess ? e : blk.alloc((size_t)(cap + 255u) / 256u + 1);
    }
  } halton;
  DevBuf<float> filterTable, aosSamples;
  DevBuf<float> prt;  // diffuse PRT: the transfer coefficients of every slot, [Terms(lmax)][cap]
  // guide renders (dr_render_guides*): the side planes k_guides writes, [3 * channels][guidesCap] floats -- a guide render's
  // channels and batch capacity; never sized by another render
  DevBuf<float> guides;
  uint32_t guidesCap = 0;
  DevBuf<uint32_t> gprtBits, gprtMark;  // glossy PRT: one visibility bit per ray and slot, [max(1, nSamples / 32)][cap], and the slots that hit, [cap]
  int spillGrid = 0;
  size_t bytes() const {  // device memory held right now (dr_scene_workspace_bytes): every buffer above
    return tiles.bytes() + scr.bytes() + genState.bytes() + tail.bytes() + tailOff.bytes() + activeA.bytes() + activeB.bytes() + closestQ.bytes() +
           anyQ.bytes() + counters.bytes() + spill.bytes() + envQ.bytes() + alive.bytes() + roundA.bytes() + roundB.bytes() + specFrames.bytes() +
           specSp.bytes() + pix.bytes() + adaptList.bytes() + adaptCount.bytes() + halton.idx.bytes() + halton.keyPix.bytes() + halton.blk.bytes() +
           filterTable.bytes() + aosSamples.bytes() + prt.bytes() + gprtBits.bytes() + gprtMark.bytes() + guides.bytes();
  }
};

// Where things live in Workspace::counters -- the only place that knows:
//   [0, 4 * stagePitch): a stage's four queue counts (active out, closest, any, shade work), one row per kind, stagePitch words
//                        apart: every wave adds to all four in one round trip (stage_flush), and same-line atomics serialise;
//   the round words:     DirectLighting over mirror / glass, the counts of the two round lists and of k_shade_spec's two unused queues;
//   [workBase, envBase): 8 per-XCD work counters per trace launch, DR_WORK_STRIDE words apart;
//   [envBase, total):    the counts of k_env's lists, one cache line per stage.
struct CounterLayout {
  struct Range { uint32_t offset, length; };
  static constexpr uint32_t stagePitch = 248;
  static constexpr uint32_t stageCount(int j, int stage) { return stagePitch * (uint32_t)j + (uint32_t)stage; }
  static constexpr uint32_t roundBase = 1008;
  static constexpr uint32_t roundNext(int round) { return roundBase + (uint32_t)(round & 1); }
  static constexpr uint32_t roundClosest = roundBase + 2, roundAny = roundBase + 3, roundEnd = roundBase + 4;
  static constexpr uint32_t workBase = 1024, workPitch = 8 * DR_WORK_STRIDE, maxLaunches = 400;
  static constexpr uint32_t workCounters(int launch) { return workBase + workPitch * (uint32_t)launch; }
  static constexpr uint32_t envBase = workBase + workPitch * maxLaunches, envPitch = 64, maxEnvStages = 256;
  static constexpr uint32_t envCount(int stage) { return envBase + envPitch * (uint32_t)stage; }
  static constexpr uint32_t total = envBase + envPitch * maxEnvStages;
  // A new round of the stage loop clears these.  Not the round words: the previous round's counts are still being read.
  static constexpr Range roundReset[2] = {{0, 1000}, {workBase, total - workBase}};
  // stages of a render at most: a row of stage counts each, and 1 + 2 * nStages trace launches
  static constexpr int maxStages() { return (int)std::min(stagePitch, (maxLaunches - 1) / 2); }
};
static_assert(CounterLayout::stageCount(3, 0) + CounterLayout::stagePitch <= CounterLayout::roundReset[0].offset + CounterLayout::roundReset[0].length,
              "the four stage rows lie inside the first reset range");
static_assert(CounterLayout::roundReset[0].offset + CounterLayout::roundReset[0].length <= CounterLayout::roundNext(0), "a new round keeps the round words");
static_assert(CounterLayout::roundEnd <= CounterLayout::workBase && CounterLayout::roundReset[1].offset == CounterLayout::workBase, "round words below the work counters");
static_assert(CounterLayout::workCounters(CounterLayout::maxLaunches) == CounterLayout::envBase, "work counters end where k_env's counts begin");
static_assert(CounterLayout::envCount(CounterLayout::maxEnvStages) == CounterLayout::total &&
                  CounterLayout::roundReset[1].offset + CounterLayout::roundReset[1].length == CounterLayout::total, "k_env's counts end the buffer");
static_assert(CounterLayout::maxStages() <= (int)CounterLayout::maxEnvStages, "every stage has a k_env count");

// What a timed pair of events measured (DrScene::TraceEv, folded into DrRenderStats by DrScene::foldEvents).
enum class TimedKind : int {
  Closest = 0,         // a closest-hit traversal launch
  Any = 1,             // an any-hit traversal launch
  Shade = 2,
  Gen = 3,             // sample generation + raygen
  Film = 4,
  Pilot = 5,           // the calibration batches as a whole (DrRenderStats.pilot_ms)
  CoherentCamera = 6,  // k_trace_pk: part of the closest-hit time, and the pk* figures
  Guides = 7,          // k_guides (a guide render's one launch per batch): part of the shading time
};

}  // namespace dr_host

struct DrScene {
  template <class T>
  using DevBuf = dr_host::DevBuf<T>;
  using Workspace = dr_host::Workspace;
  using TimedKind = dr_host::TimedKind;
  DScene d;
  DevBuf<uint4> nodes, pairs;
  DevBuf<float4> tris, mats, shtris;
  DevBuf<DLight> lights;
  DevBuf<DLightTri> ltris;
  DevBuf<DQuadric> quads;
  std::vector<DQuadric> hostQuads;
  DevBuf<float4> srec;
  DevBuf<float> xforms;
  DevBuf<float> lcdf;
  DevBuf<float> envTexels, envCondFunc, envCondCdf, envCondInt, envMargFunc, envMargCdf;
  DevBuf<uint16_t> envCondGuide;
  DevBuf<TraceCounters> ctr;
  uint32_t bvhDepth = 0;
  bool traceCalibrated = false;
  uint32_t bigRenders = 0;      // big renders this scene has finished (planBatches: the first one keeps its batches at 2^27 slots)
  int stateLayout = 0;          // path-state layout of this scene's path renders: 0 = not measured yet, 64 / 4 (LayoutOps)
  float layoutDensity = -1.f;   //   what decided it: the share of a pilot batch's slots still alive at the second bounce
  float calibMs[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};  // pilot of dr_render_device: [closest / any][v2 / v3 / v3c] ms
  float calibFarFirst = 0.f;  // any-hit rays, far child first over the reference order: time per ray of k_trace<1> in the pilot's first two batches (0 = not measured)
  float calibPerGB[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};  //   the same as ms per algorithmic GB (what the choice compares; 0 = not measured)
  // what the last dr_render_device call actually ran with (dr_scene_last_render_info): state layout, the traversal kernels of
  // its last batch, a reserved word (-1), calibration batches, workgroups per CU
  int32_t lastInfo[8] = {0, 0, 0, -1, 0, 0, 0, 0};
  uint32_t adaptiveN = 0;  // dr_scene_get_adaptive_pixels: entries of ws.adaptList the last render left (0 after any other sampler's render)
  std::vector<int32_t> lightNSamples;
  // diffuse PRT: per material DrMaterial.type, or -1 for a matte material with sigma != 0 (Oren-Nayar) -- what planRender refuses by
  // name; and the incident-light coefficients of the last lmax asked for (prtIncident: c_in[Terms(lmax)][3], the K table; lmax 0: none yet)
  std::vector<int32_t> prtMaterials;
  struct {
    DevBuf<double> K;
    DevBuf<float> cin;
    int lmax = 0;
    uint32_t after[2] = {0u, 0u};  // the two randomUint() of the preprocess RNG behind the lights' draws: ComputeBSDFMatrix's scramble
  } prt;
  // glossy PRT: Kd, Ks, roughness (dr_scene_set_glossy_prt; the reference's defaults until then) and the BSDF matrix
  // B[Terms][Terms][3] of the key (lmax, ns, Kd, Ks, roughness) it was last computed for (gprtBsdfMatrix; lmax 0: none yet)
  struct {
    float Kd[3] = {0.5f, 0.5f, 0.5f}, Ks[3] = {0.25f, 0.25f, 0.25f};
    double roughness = 0.1;
    DevBuf<float> B;
    int lmax = 0, ns = 0;
    float keyKd[3] = {0.f, 0.f, 0.f}, keyKs[3] = {0.f, 0.f, 0.f};
    double keyRoughness = 0.0;
  } gprt;
  // radiance probes: the grid dr_scene_set_probes attached -- lmax (0: none), includeDirectInProbes, nProbes, the bounds, the
  // coefficients c_in[cell][Terms(lmax)][3] and the K table on the device -- which a DR_INTEGRATOR_USE_PROBES render reads
  struct {
    DevBuf<double> K;
    DevBuf<float> cin;
    int lmax = 0, includeDirect = 0, n[3] = {0, 0, 0};
    float b[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  } probes;
  bool hasSpecular = false;  // some material is a mirror / glass
  bool hasDeltaLight = false;
  // DirectLighting sample layout (direct_lighting_integrator.dart:70-87), fixed by the lights' nsamples
  DevBuf<LdBlock> dlBlocks;
  DevBuf<DirectStage> dlStages;
  int dlNBlocks = 0, dlNStages = 0, dlNFloats = 0, dlN1D = 0;
  bool dlMulti = false;
  Workspace ws;
  hipStream_t s3 = nullptr;  // the any-hit launches of a stage, beside the closest-hit ones
  // stats of the last render
  DrRenderStats stats;
  // after: set for an any-hit launch that ran beside the stage's closest-hit launch (its end): only the time AFTER that
  // counts as any-hit time
  struct TraceEv { hipEvent_t e0, e1; TimedKind kind; hipEvent_t after = nullptr; };
  std::vector<TraceEv> traceEvents;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> renderEvents;
  std::vector<hipEvent_t> eventPool;
  size_t eventsUsed = 0;
  bool statsPending = false;
  hipEvent_t lastEvent = nullptr;
  // dr_scene_get_coherent_stats: what k_trace_pk traced of the closest-hit totals since the last dr_reset_stats
  double pkMs = 0.0;
  uint64_t pkLaunches = 0;
  unsigned long long pkRays = 0, pkNodes = 0, pkTris = 0;
  // dr_scene_get_sampler_stats: (pixel, LD block) pairs the device sampler shuffled / that the path's reads name (rp.genMask), since the
  // last dr_reset_stats (lazy generation: the first is smaller where paths end early -- sky pixels)
  unsigned long long genDone = 0, genDoneHost = 0, genNamed = 0;
  // Timings of finished launches are folded into `stats` and their events recycled, so a long-lived scene (a frame
  // loop calling dr_render_device) does not grow the pool or the lists without bound.
  void foldEvents() {
    for (auto& ev : traceEvents) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev.after ? ev.after : ev.e0, ev.e1) != hipSuccess) continue;
      if (t < 0.f) t = 0.f;  // (an any-hit launch that ended before the closest-hit one beside it)
      switch (ev.kind) {  // (no default: -Wall names a kind this forgets)
        case TimedKind::Any: stats.any_ms += t; stats.any_launches++; break;
        case TimedKind::Closest: stats.closest_ms += t; stats.closest_launches++; break;
        case TimedKind::CoherentCamera: stats.closest_ms += t; stats.closest_launches++; pkMs += t; pkLaunches++; break;  // k_trace_pk: part of the closest-hit time
        case TimedKind::Shade: case TimedKind::Guides: stats.shade_ms += t; break;
        case TimedKind::Gen: stats.gen_ms += t; break;
        case TimedKind::Pilot: stats.pilot_ms += t; break;
        case TimedKind::Film: stats.film_ms += t; break;
      }
    }
    for (auto& ev : renderEvents) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) stats.total_ms += t;
    }
    stats.trace_ms = stats.closest_ms + stats.any_ms;
    stats.trace_launches = stats.closest_launches + stats.any_launches;
    traceEvents.clear();
    renderEvents.clear();
    eventsUsed = 0;
  }
  hipEvent_t getEvent() {
    if (eventsUsed == eventPool.size()) {
      hipEvent_t e;
      (void)hipEventCreate(&e);
      eventPool.push_back(e);
    }
    return eventPool[eventsUsed++];
  }
  ~DrScene() {
    (void)hipDeviceSynchronize();  // nothing of this scene may still be in flight when its buffers and events go away
    for (auto e : eventPool) (void)hipEventDestroy(e);
    if (s3) (void)hipStreamDestroy(s3);
  }
};

namespace dr_host {

// How the sample vectors of one render are stored (see BatchState)
struct SampleForm {
  bool compact;
  int nFloats, nBlocks, idxShift;
  int svWords() const { return compact ? ((nBlocks * 64) << idxShift) / 4 : 64 * nFloats; }
};

// The kernels that read or write the path state exist twice: the default layout (every field of a tile's 64 slots one
// 256-byte run) and sp4 (sub-tiles of four slots: a slot's 41 words within 656 contiguous bytes; the same sources compiled
// with -DDR_SUB=4 -DDR_NS=sp4).  Dense stage lists are faster in the first; lists that thin out early -- open scenes under an
// environment map, where most bounce rays leave -- in the second (C5: shade 711 -> 536 ms, MEASUREMENTS.md round 3).
// A render picks one (dr_render_device); results do not depend on it.
// X(member, function) for every launcher a layout has its own copy of: LayoutOps' members and both tables (dr_api.hip) are this list
#define DR_LAYOUT_LAUNCHERS(X)                                                                                                          \
  X(trace, launch_trace) X(trace_coherent, launch_trace_coherent) X(trace_kernel_id, trace_kernel_id) X(gen_samples, launch_gen_samples)   \
  X(gen_strat, launch_gen_strat) X(export_samples, launch_export_samples) X(adaptive_decide, launch_adaptive_decide)                       \
  X(halton_select, launch_halton_select) X(gen_halton, launch_gen_halton) X(gen_random, launch_gen_random) X(mark_alive, launch_mark_alive)   \
  X(sum_alive, launch_sum_alive) X(transpose_samples, launch_transpose_samples) X(raygen, launch_raygen) X(shade_path, launch_shade_path)   \
  X(env, launch_env) X(shade_direct, launch_shade_direct) X(shade_spec, launch_shade_spec) X(shade_whitted, launch_shade_whitted)          \
  X(shade_ao, launch_shade_ao) X(shade_feature, launch_shade_feature) X(shade_prt, launch_shade_prt) X(shade_gprt, launch_shade_gprt) X(gprt_finish, launch_gprt_finish) X(shade_probes, launch_shade_probes) X(shade_material, launch_shade_material) X(film, launch_film) \
  X(guides, launch_guides) X(guide_plane, launch_guide_plane)
struct LayoutOps {
#define DR_LAYOUT_MEMBER(member, fn) decltype(&fn) member;
  DR_LAYOUT_LAUNCHERS(DR_LAYOUT_MEMBER)
  int stateWords;  // 4-byte words of fixed path state per slot in this layout (a tile is 64 of them + the sample region):
                   // what the kernels' own translation unit was compiled with (layout_state_words), not a constant repeated here
};
extern const LayoutOps kLayout64, kLayoutSp4;  // dr_api.hip

// The sampler modes of the C ABI (DrRenderDesc.sampler_mode) as the planner sees them, and what each one declares: every decision of
// dr_plan.hip / dr_api.hip / dr_batch.hip that depends on the mode reads one of these facts.  A new mode adds a row, its case in planSampler (its
// own rules), its function in planPixelSource where its pixels come from somewhere new (dr_plan.hip), and its case in genSamples.
enum class SamplerKind : int { HostBuffer, LowDiscrepancy, Stratified, Adaptive, Halton, Random };
struct SamplerTraits {
  bool deviceGenerated;  // the device sampler runs (else the caller's vectors are uploaded per batch)
  bool floatForm;        // sample vectors are floats; the other kinds use the compact form unless rp.blocks forces floats
  bool pixelBound;       // samples belong to a pixel list known up front (uploaded once, film_samples, tiles, one-batch slack, coherent camera, pilot); else written per batch
  bool pow2Spp;          // spp is a power of two (the slot -> pixel maps of the batches are shifts)
  const char* identityRoundSize;  // where Sampler.roundSize is the identity a light's nsamples must be its own rounding: the refusal's text, else null
};
constexpr SamplerTraits kSamplerTraits[] = {
    {false, true, true, true, nullptr},       // HostBuffer
    {true, false, true, true, nullptr},       // LowDiscrepancy
    {true, true, true, true, "stratified sampler: a light's nsamples must be a power of two (StratifiedSampler.roundSize is the identity, the scene's sample layout is the rounded one)"},  // Stratified
    {true, false, true, true, nullptr},       // Adaptive
    {true, true, false, false, "halton sampler: a light's nsamples must be a power of two (HaltonSampler.roundSize is the identity, the scene's sample layout is the rounded one)"},  // Halton
    {true, true, true, true, "random sampler: a light's nsamples must be a power of two (RandomSampler.roundSize is the identity, the scene's sample layout is the rounded one)"}};  // Random

// The surface integrators of the C ABI (DrRenderDesc.integrator) as the planner sees them, and what each one declares: every decision of
// dr_plan.hip / dr_api.hip / dr_batch.hip that depends on the integrator reads one of these facts or is a case of a switch over the kind (planStages,
// sideBufferBytesPerSlot / allocSideBuffers, BatchRunner::stage's launcher and rays, lastInfoWord).  A new integrator adds a row, its cases -- in planStages
// a call of its own plan function where it has rules (dr_plan.hip) --, its launcher in DR_LAYOUT_LAUNCHERS.
// The kinds ARE the ABI's values.  (No kind 6, 8, 10, 12: the ABI leaves those values unassigned -- see DR_INTEGRATOR_DIFFUSE_PRT in dartray_hip.h -- and
// knownIntegrator refuses them like any other unknown value.)
enum class IntegratorKind : int {
  DirectAll = DR_INTEGRATOR_DIRECT_ALL, Path = DR_INTEGRATOR_PATH, DirectOne = DR_INTEGRATOR_DIRECT_ONE, Whitted = DR_INTEGRATOR_WHITTED,
  AmbientOcclusion = DR_INTEGRATOR_AO, Feature = DR_INTEGRATOR_FEATURE, DiffusePRT = DR_INTEGRATOR_DIFFUSE_PRT, GlossyPRT = DR_INTEGRATOR_GLOSSY_PRT,
  UseProbes = DR_INTEGRATOR_USE_PROBES, Material = DR_INTEGRATOR_MATERIAL
};
struct IntegratorTraits {
  bool assigned;         // the row's index names an integrator (else: a value the ABI leaves unassigned, kUnassignedIntegratorRow)
  bool sceneSlots;       // the sample slots are the scene's DirectLighting layout (the lights' nsamples decide: dlN1D / dlNFloats / dlBlocks), n1D / n2D unused
  int n1D, n2D;          // else: the 1-D and 2-D slots behind the five camera floats, the volume integrator's tau + scatter among the 1-D ones
  bool pathStages;       // k_shade_path's stages, max_depth + 2 of them: deferred NEE, RNG draws beyond the sample vector, the blocks the path reads
                         //   (genMask, lazy generation), k_env, the layout pilot and the sparse default layout
  bool specularRounds;   // mirror / glass recurse through k_shade_spec: one round of the stage loop per vertex of a slot's ray tree
  const char* depthBelowOne;  // max_depth counts the camera vertex, so it is at least 1: the refusal's text, else null
  const char* adaptive;       // the adaptive sampler is not supported: the refusal's text, else null
};
// The row of a value inside the table's range that names no integrator: never read -- knownIntegrator says no -- and spelt as DirectAll, which an
// unknown value counts as.  An integrator added later takes the value behind the last one, not one of these: what the library answers for them is
// pinned behaviour (tests/test_feature_integrator.py, test_prt_integrator.py, test_glossy_prt_integrator.py, test_probes_integrator.py, test_guides.py)
constexpr IntegratorTraits kUnassignedIntegratorRow = {false, true, 0, 0, false, false, nullptr, nullptr};
constexpr IntegratorTraits kIntegratorTraits[] = {
    {true, true, 0, 0, false, true, nullptr, nullptr},    // DirectAll: per light a light and a BSDF slot pair of roundSize(nsamples) entries (2n + 2 and 2n slots at nsamples 1)
    {true, false, 14, 9, true, false, nullptr, nullptr},  // Path: 3 x (light 1D+2D, lightNum 1D, bsdf 1D+2D, path 1D+2D) + tau + scatter
    // DirectOne (direct_lighting_integrator.dart:82-87): light component, lightNum, BSDF component + tau + scatter; light position, BSDF direction
    {true, false, 5, 2, false, true, nullptr, nullptr},
    // Whitted (whitted_integrator.dart:26-72): no requestSamples -- tau + scatter only; one stage per light, any-hit rays only
    {true, false, 2, 0, false, true, "whitted integrator: max_depth must be at least 1 (maxdepth counts the camera vertex: ray.depth + 1 < maxDepth)",
     "whitted integrator: the adaptive sampler is not supported (its second pass over the rounds of the specular recursion has no test; every other sampler mode is)"},
    // AmbientOcclusion (ambient_occlusion_integrator.dart:28-53): no requestSamples -- tau + scatter only; one any-hit ray per stage,
    // nsamples of them per camera hit in rounds of the stage loop; max_depth is not read
    {true, false, 2, 0, false, false, nullptr,
     "ambient occlusion integrator: the adaptive sampler is not supported (its second pass over the rounds of occlusion rays has no test; every other sampler mode is)"},
    // Feature (no reference class): no requestSamples -- tau + scatter only; one stage, no ray beyond the camera's; max_depth and
    // the lights are not read
    {true, false, 2, 0, false, false, nullptr, "feature integrator: the adaptive sampler is not supported"},
    kUnassignedIntegratorRow,  // (6)
    // DiffusePRT (diffuse_prt_integrator.dart:42-81): an empty requestSamples -- tau + scatter only; one any-hit ray per stage, nsamples of
    // them per camera hit in rounds of the stage loop, as for AmbientOcclusion; max_depth is not read
    {true, false, 2, 0, false, false, nullptr,
     "diffuse PRT: the adaptive sampler is not supported (its second pass over the rounds of occlusion rays has no test; every other sampler mode is)"},
    kUnassignedIntegratorRow,  // (8)
    // GlossyPRT (glossy_prt_integrator.dart:53-116): an empty requestSamples -- tau + scatter only; DiffusePRT's stages and rounds,
    // then one finish launch per batch; max_depth is not read
    {true, false, 2, 0, false, false, nullptr,
     "glossy PRT: the adaptive sampler is not supported (its second pass over the rounds of occlusion rays has no test; every other sampler mode is)"},
    kUnassignedIntegratorRow,  // (10)
    // UseProbes (use_probes_integrator.dart:74-88): requestSamples asks for the scene's DirectLighting "all" slots although Li never
    // reads them (the grid includes the direct light); one stage, no ray beyond the camera's; max_depth is not read
    {true, true, 0, 0, false, false, nullptr, "use probes: the adaptive sampler is not supported (its second pass has no test under this integrator; every other sampler mode is)"},
    kUnassignedIntegratorRow,  // (12)
    // Material (no reference class): the feature integrator's row -- no requestSamples, tau + scatter only; one stage, no ray beyond
    // the camera's; max_depth is not read
    {true, false, 2, 0, false, false, nullptr, "material integrator: the adaptive sampler is not supported"}};
// The one check of the table against the ABI: 14 rows, and the assigned ones are exactly the ten DR_INTEGRATOR_* values (the kinds)
constexpr bool integratorTableMatchesAbi() {
  constexpr IntegratorKind kinds[] = {IntegratorKind::DirectAll, IntegratorKind::Path, IntegratorKind::DirectOne, IntegratorKind::Whitted, IntegratorKind::AmbientOcclusion,
                                      IntegratorKind::Feature, IntegratorKind::DiffusePRT, IntegratorKind::GlossyPRT, IntegratorKind::UseProbes, IntegratorKind::Material};
  constexpr int rows = sizeof(kIntegratorTraits) / sizeof(kIntegratorTraits[0]);
  int assigned = 0;
  for (int v = 0; v < rows; ++v) assigned += kIntegratorTraits[v].assigned ? 1 : 0;
  for (IntegratorKind k : kinds)
    if ((int)k < 0 || (int)k >= rows || !kIntegratorTraits[(int)k].assigned) return false;
  return rows == 14 && assigned == 10;
}
static_assert(integratorTableMatchesAbi(), "kIntegratorTraits is indexed by DrRenderDesc.integrator: a row per value up to the last DR_INTEGRATOR_*, the unassigned ones placeholders");
inline bool knownIntegrator(int32_t v) { return v >= 0 && v < (int32_t)(sizeof(kIntegratorTraits) / sizeof(kIntegratorTraits[0])) && kIntegratorTraits[v].assigned; }

// The feature integrator's refusals (dr_feature_check, planRender): null, or the text and its code
inline const char* featureRefusal(int32_t channel, uint64_t nprims, int* code) {
  if (channel < DR_FEATURE_NG || channel > DR_FEATURE_ID) {
    *code = DR_ERR_INVALID;
    return "feature integrator: unknown channel (DR_FEATURE_NG, _NS, _DEPTH, _UV or _ID)";
  }
  if (channel == DR_FEATURE_ID && nprims >= (1ull << 24)) {
    *code = DR_ERR_UNSUPPORTED;
    return "feature integrator: the id channel needs a scene of fewer than 2^24 primitives (an index + 1 must be exact in the film's f32)";
  }
  return nullptr;
}

// The material integrator's refusal (dr_material_check, planRender): null, or the text
inline const char* materialRefusal(int32_t channel) {
  if (channel != DR_MATERIAL_CHANNEL_ALBEDO && channel != DR_MATERIAL_CHANNEL_EMISSION)
    return "material integrator: unknown channel (DR_MATERIAL_CHANNEL_ALBEDO or _EMISSION)";
  return nullptr;
}

// The refusals of a guide render (dr_render_guides_check, dr_render_guides*): null, or the text and its code.  The integrators that
// own their camera stage through a kernel of the four below the seam -- Path, DirectLighting "all" and "one", Whitted, ambient occlusion -- are
// served; every other one is refused by name, and so is the adaptive sampler, which the feature integrator refuses too
inline const char* guidesRefusal(const DrRenderDesc* rd, const DrGuidesDesc* g, uint64_t nprims, int* code) {
  *code = DR_ERR_INVALID;
  if (!rd || !g) return "render guides: null argument";
  if (!knownIntegrator(rd->integrator)) return "render guides: unknown integrator";
  *code = DR_ERR_UNSUPPORTED;
  switch ((IntegratorKind)rd->integrator) {  // (no default: -Wall names a kind this forgets)
    case IntegratorKind::DirectAll: case IntegratorKind::Path: case IntegratorKind::DirectOne: case IntegratorKind::Whitted:
    case IntegratorKind::AmbientOcclusion: break;
    case IntegratorKind::Feature: return "render guides: the feature integrator is not supported (its image is a guide already: render it as it is)";
    case IntegratorKind::DiffusePRT: return "render guides: the diffuse PRT integrator is not supported (guides beside its side buffer have no test)";
    case IntegratorKind::GlossyPRT: return "render guides: the glossy PRT integrator is not supported (guides beside its side buffers have no test)";
    case IntegratorKind::UseProbes: return "render guides: the use probes integrator is not supported (guides under it have no test)";
    case IntegratorKind::Material: return "render guides: the material integrator is not supported (its image is a guide already: render it as it is)";
  }
  if (rd->sampler_mode == DR_SAMPLER_ADAPTIVE) return "render guides: the adaptive sampler is not supported (the feature integrator refuses it; a second pass would write its guides twice)";
  *code = DR_ERR_INVALID;
  if (g->count < 1) return "render guides: the channel list is empty (count must be 1 to 5)";
  if (g->count > DR_GUIDES_MAX) return "render guides: more than five channels (count must be 1 to 5)";
  for (int i = 0; i < g->count; ++i) {
    if (g->channels[i] < DR_FEATURE_NG || g->channels[i] > DR_FEATURE_ID) return "render guides: unknown channel (DR_FEATURE_NG, _NS, _DEPTH, _UV or _ID)";
    for (int j = 0; j < i; ++j)
      if (g->channels[j] == g->channels[i]) return "render guides: a channel is given twice (every DR_FEATURE_* value at most once)";
  }
  for (int i = 0; i < g->count; ++i)
    if (g->channels[i] == DR_FEATURE_ID && nprims >= (1ull << 24)) {
      *code = DR_ERR_UNSUPPORTED;
      return "render guides: the id channel needs a scene of fewer than 2^24 primitives (an index + 1 must be exact in the film's f32)";
    }
  return nullptr;
}

// An integrator's sample slots; the floats of a sample vector are computed here and nowhere else.
struct SlotCounts {
  int n1D, n2D;
  int nFloats() const { return 5 + n1D + 2 * n2D; }
};
// sc null: DirectAll as of nlights lights of nsamples 1
inline SlotCounts integratorSlots(IntegratorKind k, const DrScene* sc, uint32_t nlights) {
  const IntegratorTraits& t = kIntegratorTraits[(int)k];
  if (!t.sceneSlots) return {t.n1D, t.n2D};
  return sc ? SlotCounts{sc->dlN1D, (sc->dlNFloats - 5 - sc->dlN1D) / 2} : SlotCounts{2 * (int)nlights + 2, 2 * (int)nlights};
}

// The rays of an integrator that sends one any-hit ray per stage (ambient occlusion, diffuse and glossy PRT): nSamples = RoundUpPow2(requested) rays per
// camera hit.  A render holds at most CounterLayout::maxStages() stages, so the rays go in rounds of the stage loop, 128 to a round (a power of two: it
// divides every larger nSamples): perRound of them in each of `rounds` rounds.
struct Rounds {
  int nSamples = 0, perRound = 0, rounds = 0;
  static Rounds of(int requested) {  // 1 <= requested <= 4096 (the plan functions refuse every other count by name)
    Rounds r;
    for (r.nSamples = 1; r.nSamples < requested;) r.nSamples <<= 1;  // RoundUpPow2 (common.dart:117-125)
    r.perRound = std::min(r.nSamples, 128);
    r.rounds = r.nSamples / r.perRound;
    return r;
  }
};

struct RenderPlan {
  DrScene* sc = nullptr;
  const DrRenderDesc* rd = nullptr;
  float* film = nullptr;
  hipStream_t s = nullptr;
  RenderParams rp;
  SampleForm sf;
  const LayoutOps* L = nullptr;  // state layout of the NEXT batch (the layout pilot decides it after the first calibration batch)
  int spp = 0;
  IntegratorKind integrator = IntegratorKind::Path;
  const IntegratorTraits* integ = &kIntegratorTraits[(int)IntegratorKind::Path];
  bool dlSpec = false, envStage = false, packedTail = false;  // dlSpec: k_shade_spec's rounds run (integ->specularRounds over a scene with mirror / glass)
  SamplerKind sampler = SamplerKind::LowDiscrepancy;
  const SamplerTraits* traits = &kSamplerTraits[(int)SamplerKind::LowDiscrepancy];
  struct { int x = 0; } strat;  // Stratified: xPixelSamples (yPixelSamples = spp / x)
  // Adaptive: two counter-mode passes.  This plan is the first (spp, rp, sf: every pixel at min; its batches end with k_adaptive_decide), secondPass()
  // derives the flagged pixels' at max.  pass: 0 = another sampler, 1 / 2 = which pass this plan runs; pixCap: pixels of a second-pass batch at most (planBatches)
  struct { int pass = 0, min = 0, max = 0; uint32_t pixCap = 0; } adaptive;
  // Halton: a "pixel" of this plan is an INDEX of the task's sequence (npixTotal = wanted, spp = 1: one slot per accepted sample); a
  // batch is a range of indices, selected on the device before it runs.  win: the task's window: left, top, right, bottom (inclusive), delta = max(width, height)
  struct { int32_t win[5] = {0, 0, 0, 0, 0}; } halton;
  // AmbientOcclusion, DiffusePRT, GlossyPRT: the running integrator's occlusion rays in rounds of the stage loop (a round is perRound + 1 stages);
  // every other integrator: none, zeros
  Rounds rounds;
  int shadowRounds() const { return rounds.rounds; }  // rounds of one-ray stages (else 0)
  struct { double minDist = 0.0, maxDist = 0.0; } ao;  // AmbientOcclusion: the rays' extent
  struct { int channel = 0; } feature;  // Feature: DR_FEATURE_*
  struct { int channel = 0; } material;  // Material: DR_MATERIAL_CHANNEL_*
  // A guide render (dr_render_guides_device): n channels (0: none, every other render), the set as k_guides' mask, and per
  // requested channel its film and its side plane (its rank in the mask).  The side planes cap the batch (sideBufferBytesPerSlot) and are sized by allocSideBuffers
  struct { int n = 0; uint32_t mask = 0u; float* film[DR_GUIDES_MAX] = {}; int plane[DR_GUIDES_MAX] = {}; } guides;
  struct { int lmax = 0; } prt;              // DiffusePRT
  struct { int lmax = 0, words = 0; } gprt;  // GlossyPRT: words of visibility bits per slot
  // the device sampler's launches for one batch (BatchRunner::loadSamples, the two sample dumps)
  void genSamples(const RenderParams& rpB, const BatchState& st, uint32_t np) const;
  // what the workspace is sized for (prepareRender): this plan's batches; adaptive: both passes'
  uint32_t wsCap = 0, wsPix = 0;
  SampleForm wsSf;
  int needTail = 0;       // RNG draws a path can make beyond the sample vector (host-buffer mode: the recorded tail)
  bool layoutKnown = false;
  int maxStateWords = 0;  // words per slot the workspace is sized for (both layouts while the layout is not known)
  bool coherentCamera = false, lazyGen = false, overlapAny = false;
  bool calibrateTrace = false, measureLayout = false;
  int pilotSets = 0;      // calibration batches: warm-up, k_trace timed, k_trace3 timed, k_trace3c timed; the layout alone: one
  size_t calibPix = 0;    // pixels per calibration batch: the first pilotSets * calibPix entries of `pixels`
  std::vector<int2> pixels;
  size_t npixTotal = 0;
  uint64_t filmSamples = 0;
  uint32_t pixPerBatch = 0, cap = 0;
  uint64_t nBatches = 0;
  int tgrid = 0, sgrid = 0, nStages = 0;
  bool calibrate() const { return calibrateTrace || measureLayout; }
};

// The calibration batches of a scene's first big render (prepareRender decided that there are some): part of the render -- nothing is
// traced twice -- and the measurement that picks the state layout and, per ray kind, the traversal kernel.
struct PilotResult {
  int setsRun = 0;
  double perByte[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // [closest / any][k_trace / k_trace3 / k_trace3c]: ms per algorithmic GB
  float ms[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  // any-hit rays of the first two batches, both through k_trace<1>: batch 0 far child first, batch 1 in the reference order
  double anyMsPerRayFar = 0.0, anyMsPerRayRef = 0.0;
};

// ---- what the units call across files ----
BatchState makeState(Workspace& w, const SampleForm& sf, const int2* pix, uint32_t nslots, bool useTail, int stateWords);  // dr_api.hip
uint64_t sideBufferBytesPerSlot(const RenderPlan& P);  // dr_api.hip: what the integrator's side buffers add to a slot (beside allocSideBuffers)
int planRender(RenderPlan& P);                                                                                              // dr_plan.hip
int planBatches(RenderPlan& P);                                                                                             // dr_plan.hip
RenderPlan secondPass(const RenderPlan& P, uint32_t nFlagged);                                                              // dr_plan.hip
bool lazyGenFor(const RenderPlan& P);                                                                                       // dr_plan.hip
void rp_film(RenderParams& rp, const DrFilm& f);                                                                            // dr_plan.hip
void enumeratePixels(const RenderParams& rp, const DrRenderDesc* rd, std::vector<int2>& pixels);                            // dr_plan.hip
int runBatches(RenderPlan& plan, const int2* pixDev, size_t firstPixel);                                                    // dr_batch.hip
int runPilot(RenderPlan& P, PilotResult& R);                                                                                // dr_batch.hip
// DR_SAMPLER_HALTON: the accepted indices of [k0, k0 + n) into the workspace (halton.idx), their number read back (the mode's host wait)
int haltonSelect(RenderPlan& P, uint64_t k0, uint32_t n, uint32_t* accepted);                                               // dr_batch.hip
int runHaltonBatches(RenderPlan& P, uint64_t* acceptedTotal);                                                               // dr_batch.hip

}  // namespace dr_host

#endif
