// dr_api.hip -- the C ABI of include/dartray_hip.h: options, what a planned render needs on the device (prepareRender), film, statistics and
// every entry point but dr_scene_create / dr_scene_destroy (dr_scene_build.hip).  A render is planned in dr_plan.hip and its batches run in
// dr_batch.hip; dr_host.h is what the four share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "dr_host.h"
#include "dr_scene_prep.h"
static_assert(DR_PREP_MAX_STACK == DR_MAX_STACK, "dr_scene_prep.h");

using namespace dr_host;

namespace {

thread_local std::string g_err;
#define DR_STATE_WORDS F_SAMPLES  // 41 4-byte words of fixed path state per slot: 3 f64 + 10 3-vectors + 5 i32

}  // namespace

namespace dr_host {

int g_device = -1;
int g_numCU = 256;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

}  // namespace dr_host

int dr_fail(int code, const std::string& msg) { return fail(code, msg); }  // for dr_comm.cpp

// ---- tuning / diagnostic switches: dr_set_option, else the environment ----
namespace {
std::mutex g_optMutex;
std::map<std::string, std::string> g_options;  // name -> value; an empty value = "unset for this process" (hides the environment's)
const char* const kOptionNames[] = {
    // what a render runs: traversal kernels, state layout, batch size, schedule, the pilot
    "DARTRAY_TRACE_IMPL", "DARTRAY_TRACE_WG_PER_CU", "DARTRAY_STATE_LAYOUT", "DARTRAY_BATCH_BITS", "DARTRAY_OVERLAP_ANY", "DARTRAY_PILOT",
    "DARTRAY_COHERENT_CAMERA",
    // the device sampler (bit-exact variants, tests)
    "DARTRAY_LAZY_GEN", "DARTRAY_GEN_ALL_BLOCKS", "DARTRAY_GEN_SLOW_DRAWS",
    // scene set-up, the collective's library, diagnostics
    "DARTRAY_SCENE_PREP", "DARTRAY_BUILD_THREADS", "DARTRAY_RCCL_LIB", "DARTRAY_STAGE_COUNTS", "DARTRAY_VERBOSE"};
static_assert(sizeof(kOptionNames) / sizeof(kOptionNames[0]) <= 15, "a new switch replaces one: measured negatives go to experiments/");

}  // namespace

DrOpt dr_opt(const char* name) {
  DrOpt o;
  {
    std::lock_guard<std::mutex> lock(g_optMutex);
    auto it = g_options.find(name);
    if (it != g_options.end()) {
      o.set = !it->second.empty();  // "" hides the environment's value
      o.value = it->second;
      return o;
    }
  }
  if (const char* e = getenv(name)) {
    o.set = true;
    o.value = e;
  }
  return o;
}

namespace {

int traceGrid() { return traceGridFor(DR_V2_WG_PER_CU); }  // the largest grid any variant launches (sizes the spill stacks)

int ensureSpill(DrScene* sc, Workspace& w, int grid) {
  // deepest stack == tree depth; the v3 kernel keeps 16 (reference, E) pairs in LDS, v2 24 references
  if (sc->bvhDepth != 0 && sc->bvhDepth <= 8) return DR_OK;
  size_t need = (size_t)grid * DR_TRACE_BLOCK * (DR_MAX_STACK - 8) * 2;  // (room for any LDS stack depth >= 8 of either variant)
  w.spillHalf = need;
  HIP_TRY(w.spill.alloc(2 * need));  // second half: the any-hit launch of a stage when it runs beside the closest-hit one
  w.spillGrid = grid;
  return DR_OK;
}

int allocWorkspace(DrScene* sc, Workspace& w, uint32_t cap, const SampleForm& sf, uint32_t pixCap, int maxTail, bool needTail, int stateWords) {
  cap = (cap + 63u) & ~63u;  // whole tiles
  if (cap > w.cap || sf.svWords() > w.svWords || stateWords > w.stateWords) {
    uint32_t c = std::max(cap, w.cap);
    int sw = std::max(sf.svWords(), w.svWords);
    w.stateWords = std::max(stateWords, w.stateWords);
    HIP_TRY(w.tiles.alloc((size_t)(c / 64) * (64 * (size_t)w.stateWords + (size_t)sw)));
    HIP_TRY(w.activeA.alloc(c));
    HIP_TRY(w.activeB.alloc(c));
    HIP_TRY(w.closestQ.alloc(2 * (size_t)c));
    HIP_TRY(w.anyQ.alloc(c));
    w.cap = c;
    w.svWords = sw;
  }
  if (sf.compact) {
    w.pixCap = std::max(w.pixCap, pixCap);
    HIP_TRY(w.scr.alloc(2 * (size_t)sf.nBlocks * w.pixCap));
    HIP_TRY(w.genState.alloc((size_t)sf.nBlocks * w.pixCap));
  }
  // (sized for THIS render's batches, not for the largest batch the workspace has ever held: a small replay after a big
  // counter-mode render would otherwise allocate cap x maxTail doubles -- 86 GB behind a C2 batch)
  if (needTail && ((size_t)cap * maxTail > w.tail.n)) HIP_TRY(w.tail.alloc((size_t)cap * maxTail));
  w.maxTail = maxTail;
  HIP_TRY(w.counters.alloc(CounterLayout::total));
  HIP_TRY(w.filterTable.alloc(256));
  return DR_OK;
}

}  // namespace

// ---- what this unit defines for the others (dr_host.h) ----
namespace dr_host {

// The two LayoutOps tables, defined once: layout_state_words() is evaluated here and nowhere else.
#define DR_LAYOUT_64(member, fn) &fn,
#define DR_LAYOUT_SP4(member, fn) &sp4::fn,
const LayoutOps kLayout64 = {DR_LAYOUT_LAUNCHERS(DR_LAYOUT_64) layout_state_words()};
const LayoutOps kLayoutSp4 = {DR_LAYOUT_LAUNCHERS(DR_LAYOUT_SP4) sp4::layout_state_words()};

BatchState makeState(Workspace& w, const SampleForm& sf, const int2* pix, uint32_t nslots, bool useTail, int stateWords) {
  BatchState st;
  st.cap = w.cap;
  st.nslots = nslots;
  st.tileStride = 64u * (uint32_t)stateWords + (uint32_t)w.svWords;  // (the layout's own words per slot: its sample region starts behind them)
  st.idxShift = (uint32_t)sf.idxShift;
  st.pix = pix;
  st.tail = useTail ? w.tail.p : nullptr;
  st.tailOff = nullptr;  // (the packed form: set per batch by dr_render_device)
  st.tailBase = 0ull;
  st.tiles = w.tiles.p;  // field offsets inside a tile: the F_* constants of dr_kernels.h
  st.svFloat = sf.compact ? 0u : 1u;
  st.svScr = sf.compact ? w.scr.p : nullptr;
  {  // (the pre-pass k_gen_burnin fills genState above 256 spp; at and below, the shuffle kernels seed and burn in their streams themselves)
    st.genState = sf.compact ? w.genState.p : nullptr;
    st.genAlive = nullptr;
    st.markAlive = nullptr;
    st.markShift = 0;
    st.padMark = 0;
  }
  st.pixCap = w.pixCap;
  st.specFrames = w.specFrames.p;
  st.specSp = w.specSp.p;
  return st;
}

void RenderPlan::genSamples(const RenderParams& rpB, const BatchState& st, uint32_t np) const {
  switch (sampler) {  // (no default: -Wall names a kind this forgets)
    case SamplerKind::HostBuffer: break;  // (the caller's vectors: BatchRunner::loadHostSamples)
    case SamplerKind::LowDiscrepancy: case SamplerKind::Adaptive: L->gen_samples(rpB, st, np, s); break;
    case SamplerKind::Stratified: L->gen_strat(rpB, st, np, strat.x, s); break;
    case SamplerKind::Halton: L->gen_halton(rpB, st, halton.win, sc->ws.halton.idx.p, sc->ws.pix.p, sc->ws.halton.keyPix.p, s); break;
    case SamplerKind::Random: L->gen_random(rpB, st, s); break;
  }
}

}  // namespace dr_host

int traceGridFor(int wgPerCU) {
  // workgroups of the persistent traversal kernels: as many as are resident at once.  v2 (k_trace): 16 KiB of stack +
  // 6 KiB of cold ray state in LDS and 72 VGPRs => 7 workgroups = 28 waves per CU; the other variants (v3: 32 KiB of
  // LDS, the quadric kernel: more registers) 6, the sixth queueing behind five where only five fit.
  wgPerCU = dr_opt("DARTRAY_TRACE_WG_PER_CU").toInt(wgPerCU);
  return g_numCU * std::max(1, std::min(wgPerCU, 8));
}

namespace dr_host {
// (dr_probes.hip traces rays of its own through launch_intersect: the grid that sizes the spill stacks, and the stacks)
int traceGridMax() { return traceGrid(); }
int ensureTraceSpill(DrScene* sc) { return ensureSpill(sc, sc->ws, traceGrid()); }
}  // namespace dr_host

extern "C" {

const char* dr_last_error(void) { return g_err.c_str(); }

int dr_set_option(const char* name, const char* value) {
  if (!name || !*name) return fail(DR_ERR_INVALID, "dr_set_option: null name");
  std::string n(name);
  for (char& c : n) c = (char)toupper((unsigned char)c);
  if (n.rfind("DARTRAY_", 0) != 0) n = "DARTRAY_" + n;
  bool known = false;
  for (const char* k : kOptionNames) known = known || n == k;
  if (!known) return fail(DR_ERR_INVALID, "dr_set_option: unknown option " + n);
  std::lock_guard<std::mutex> lock(g_optMutex);
  if (value) g_options[n] = value;  // "" hides the environment's value
  else g_options.erase(n);          // null: back to the environment's value
  return DR_OK;
}
const char* dr_version(void) { return "dartray_amd 0.6 (gfx950, abi 9)"; }
int32_t dr_abi_version(void) { return DR_ABI_VERSION; }

int dr_init(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(DR_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return fail(DR_ERR_INVALID, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  g_numCU = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // the two sets of state-touching kernels must be the two layouts this file hands out (dr_kernels.hip / dr_trace.hip are
  // compiled twice: as they are, and with -DDR_SUB=4 -DDR_NS=sp4 -DDR_STATE_WORDS_K=48 -DDR_GROUPED=1)
  if (layout_sub() != 64 || layout_state_words() != DR_STATE_WORDS || sp4::layout_sub() != 4 || sp4::layout_state_words() < DR_STATE_WORDS ||
      kLayout64.stateWords != layout_state_words() || kLayoutSp4.stateWords != sp4::layout_state_words())
    return fail(DR_ERR_UNSUPPORTED, "libdartray_hip was linked from kernel objects of unexpected state layouts");
  g_device = device;
  return DR_OK;
}

int32_t dr_sample_floats(int32_t integrator, uint32_t nlights) {
  // kIntegratorTraits' slots (dr_host.h); a value that names no integrator counts as DirectLighting "all", as ever
  return integratorSlots(knownIntegrator(integrator) ? (IntegratorKind)integrator : IntegratorKind::DirectAll, nullptr, nlights).nFloats();
}

int dr_render_guides_check(const DrRenderDesc* desc, const DrGuidesDesc* guides, uint64_t nprimitives) {
  int code = DR_OK;
  if (const char* why = guidesRefusal(desc, guides, nprimitives, &code)) return fail(code, why);
  return DR_OK;
}

int dr_feature_check(int32_t channel, uint64_t nprimitives) {
  int code = DR_OK;
  if (const char* why = featureRefusal(channel, nprimitives, &code)) return fail(code, why);
  return DR_OK;
}

int dr_material_check(int32_t channel) {
  if (const char* why = materialRefusal(channel)) return fail(DR_ERR_INVALID, why);
  return DR_OK;
}

int32_t dr_scene_sample_floats(const DrScene* scene, int32_t integrator) {
  if (!scene) return -1;
  if (!knownIntegrator(integrator)) return dr_sample_floats(integrator, scene->d.nlights);
  return integratorSlots((IntegratorKind)integrator, scene, scene->d.nlights).nFloats();  // ("all": the lights' nsamples decide)
}

int dr_scene_get_trace_kernels(const DrScene* sc, uint32_t out[2]) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  out[0] = sc->traceCalibrated ? sc->d.traceKernel[0] : 0u;
  out[1] = sc->traceCalibrated ? sc->d.traceKernel[1] : 0u;
  return DR_OK;
}

int dr_scene_last_render_info(const DrScene* sc, int32_t out[8]) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  for (int i = 0; i < 8; ++i) out[i] = sc->lastInfo[i];
  return DR_OK;
}

int dr_scene_get_pilot(const DrScene* sc, float out[6]) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  for (int c = 0; c < 3; ++c) out[c] = sc->calibPerGB[0][c];
  out[3] = sc->calibPerGB[1][0];
  out[4] = sc->calibPerGB[1][1];
  out[5] = sc->calibFarFirst;
  return DR_OK;
}

int dr_scene_set_trace_kernels(DrScene* sc, const uint32_t in[2]) {
  if (!sc || !in) return fail(DR_ERR_INVALID, "null argument");
  if (in[0] == 0u && in[1] == 0u) {
    sc->traceCalibrated = false;
    sc->d.traceKernel[0] = sc->d.traceKernel[1] = 0u;
    return DR_OK;
  }
  for (int k = 0; k < 2; ++k) {
    if (in[k] != 2u && in[k] != 3u && !(k == 0 && in[k] == 5u) && !(k == 1 && (in[k] == 6u || in[k] == 7u)))
      return fail(DR_ERR_INVALID, "trace kernel must be 2 or 3 (closest-hit rays also 5, any-hit rays also 6 / 7 = 2 / 3 far child first; or 0, 0 to measure again)");
    if (in[k] != 2u && in[k] != 6u && (!sc->d.pairs || sc->d.nquads)) return fail(DR_ERR_UNSUPPORTED, "this scene cannot use the sibling-pair kernels");
  }
  sc->d.traceKernel[0] = in[0];
  sc->d.traceKernel[1] = in[1];
  sc->traceCalibrated = true;
  return DR_OK;
}

int dr_scene_get_pairs(const DrScene* sc, void* out, uint64_t cap_bytes, uint64_t* npairs_out, uint32_t* top_pairs_out, uint32_t* depth_out) {
  if (!sc || !npairs_out) return fail(DR_ERR_INVALID, "null argument");
  *npairs_out = sc->d.pairs ? sc->d.npairs : 0;
  if (top_pairs_out) *top_pairs_out = sc->d.topPairs;
  if (depth_out) *depth_out = sc->bvhDepth;
  if (out && sc->d.pairs) {
    if (cap_bytes < (uint64_t)sc->d.npairs * 64) return fail(DR_ERR_INVALID, "pair buffer too small");
    HIP_TRY(hipMemcpy(out, sc->d.pairs, (size_t)sc->d.npairs * 64, hipMemcpyDeviceToHost));
  }
  return DR_OK;
}

int dr_scene_workspace_bytes(const DrScene* sc, uint64_t* bytes_out) {
  if (!sc || !bytes_out) return fail(DR_ERR_INVALID, "null argument");
  *bytes_out = sc->ws.bytes();
  return DR_OK;
}

int dr_scene_get_table_counts(const DrScene* sc, uint32_t out[6]) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  out[0] = sc->d.nlights;
  out[1] = sc->d.nltris;
  out[2] = sc->d.ncdf;
  out[3] = sc->d.nmats;
  out[4] = (uint32_t)sizeof(DLight);
  out[5] = (uint32_t)sizeof(DLightTri);
  return DR_OK;
}

int dr_scene_get_state_layout(const DrScene* sc, int32_t* layout_out, float* density_out) {
  if (!sc || !layout_out) return fail(DR_ERR_INVALID, "null argument");
  *layout_out = sc->stateLayout;
  if (density_out) *density_out = sc->layoutDensity;
  return DR_OK;
}

int dr_scene_set_state_layout(DrScene* sc, int32_t layout) {
  if (!sc) return fail(DR_ERR_INVALID, "null argument");
  if (layout != 0 && layout != 4 && layout != 64) return fail(DR_ERR_INVALID, "state layout must be 64 or 4 (or 0 to measure again)");
  sc->stateLayout = layout;
  if (layout == 0) sc->layoutDensity = -1.f;
  return DR_OK;
}

int dr_intersect(DrScene* sc, const DrRay* rays, int64_t n, DrHit* out, int32_t any_hit) {
  if (!sc || (n > 0 && (!rays || !out))) return fail(DR_ERR_INVALID, "null argument");
  if (n <= 0) return DR_OK;
  if (n >= (1ll << 31)) return fail(DR_ERR_INVALID, "too many rays in one call");
  int grid = std::min<int64_t>(traceGrid(), (n + DR_TRACE_BLOCK - 1) / DR_TRACE_BLOCK);
  int rc = ensureSpill(sc, sc->ws, traceGrid());
  if (rc) return rc;
  DevBuf<DrRay> dR;
  DevBuf<DrHit> dH;
  DevBuf<uint32_t> work;
  HIP_TRY(dR.alloc(n));
  HIP_TRY(dH.alloc(n));
  HIP_TRY(work.alloc(8 * DR_WORK_STRIDE));
  HIP_TRY(hipMemcpy(dR.p, rays, n * sizeof(DrRay), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(work.p, 0, 8 * DR_WORK_STRIDE * sizeof(uint32_t)));
  HIP_TRY(hipMemset(sc->ctr.p, 0, sizeof(TraceCounters)));
  launch_intersect(sc->d, dR.p, n, dH.p, any_hit, sc->ws.spill.p, work.p, sc->ctr.p, grid, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dH.p, n * sizeof(DrHit), hipMemcpyDeviceToHost));
  TraceCounters c;
  HIP_TRY(hipMemcpy(&c, sc->ctr.p, sizeof(c), hipMemcpyDeviceToHost));
  memset(&sc->stats, 0, sizeof(sc->stats));
  sc->traceEvents.clear();
  sc->renderEvents.clear();
  sc->eventsUsed = 0;
  sc->stats.closest_rays = c.closest_rays; sc->stats.any_rays = c.any_rays;
  sc->stats.closest_nodes = c.closest_nodes; sc->stats.any_nodes = c.any_nodes;
  sc->stats.closest_tris = c.closest_tris; sc->stats.any_tris = c.any_tris;
  sc->statsPending = false;
  HIP_TRY(hipMemset(sc->ctr.p, 0, sizeof(TraceCounters)));
  return DR_OK;
}

}  // extern "C"

// ===========================================================================
// dr_render_device, in units: RenderPlan (dr_host.h; what this call runs: planRender -- sampler, integrator, camera and film, stages, pixel
// source -- and planBatches: dr_plan.hip), prepareRender (workspace, the integrator's side buffers, pilot decision, uploads -- here),
// BatchRunner (one batch through the stage loop), runBatches and runPilot (the calibration batches) -- dr_batch.hip -- and the entry
// point, here, which strings them together and records what ran.
// ===========================================================================

// An integrator's side buffers, in two functions that name the same buffers: the bytes they add to a slot -- planBatches shrinks the batch by them --
// and their allocation, sized by this plan's batch capacity (P.wsCap, which planBatches shrank to fit them), not by the capacity an earlier, larger
// render left the workspace with.  (The round lists of ambient occlusion have never been counted: 8 bytes beside a slot's 200.)
uint64_t dr_host::sideBufferBytesPerSlot(const RenderPlan& P) {
  uint64_t bytes = (uint64_t)P.guides.n * 12;  // a guide render: a side plane of three floats per channel
  if (P.dlSpec) bytes += (uint64_t)std::max(1, P.rd->max_depth) * sizeof(SpecFrame) + 12;  // the slot's frames, its stack pointer + the round lists
  switch (P.integrator) {  // (no default: -Wall names a kind this forgets)
    case IntegratorKind::DirectAll: case IntegratorKind::Path: case IntegratorKind::DirectOne: case IntegratorKind::Whitted:
    case IntegratorKind::AmbientOcclusion: case IntegratorKind::Feature: case IntegratorKind::UseProbes: case IntegratorKind::Material: break;
    case IntegratorKind::DiffusePRT: bytes += (uint64_t)sh_terms(P.prt.lmax) * 4 + 8; break;  // the slot's transfer coefficients + the round lists
    case IntegratorKind::GlossyPRT: bytes += (uint64_t)P.gprt.words * 4 + 4 + 8; break;  // the slot's visibility words, its hit mark + the round lists
  }
  return bytes;
}

namespace {

// ... and, with a PRT integrator's buffers, what it computes once per scene and key before the first batch
int allocSideBuffers(RenderPlan& P) {
  DrScene* sc = P.sc;
  Workspace& w = sc->ws;
  if (P.guides.n) {  // the side planes, [3 * channels][wsCap in whole tiles]
    w.guidesCap = (P.wsCap + 63u) & ~63u;
    HIP_TRY(w.guides.alloc(3 * (size_t)P.guides.n * (size_t)w.guidesCap));
  }
  if (P.dlSpec) {
    HIP_TRY(w.specFrames.alloc((size_t)w.cap * std::max(1, P.rd->max_depth) * DR_SPEC_FRAME_WORDS));
    HIP_TRY(w.specSp.alloc(w.cap));
  }
  if (P.dlSpec || P.shadowRounds() > 1) {  // (rays in rounds: the slots that hit, handed from a round's last stage to the next round's first)
    HIP_TRY(w.roundA.alloc(w.cap));
    HIP_TRY(w.roundB.alloc(w.cap));
  }
  switch (P.integrator) {  // (no default: -Wall names a kind this forgets)
    case IntegratorKind::DirectAll: case IntegratorKind::Path: case IntegratorKind::DirectOne: case IntegratorKind::Whitted:
    case IntegratorKind::AmbientOcclusion: case IntegratorKind::Feature: case IntegratorKind::UseProbes: case IntegratorKind::Material: break;
    case IntegratorKind::DiffusePRT:  // the transfer coefficients, [Terms(lmax)][wsCap]; the incident light
      HIP_TRY(w.prt.alloc((size_t)P.wsCap * (size_t)sh_terms(P.prt.lmax)));
      return prtIncident(sc, P.prt.lmax, P.rd->camera.shutter_open, P.s);
    case IntegratorKind::GlossyPRT:  // the visibility bits and the hit marks; the incident light and the BSDF matrix (ComputeBSDFMatrix(..., 1024, lmax): glossy_prt_integrator.dart:48)
      HIP_TRY(w.gprtBits.alloc((size_t)P.wsCap * (size_t)P.gprt.words));
      HIP_TRY(w.gprtMark.alloc((size_t)P.wsCap));
      return gprtBsdfMatrix(sc, P.gprt.lmax, 1024, P.rd->camera.shutter_open, P.s);
  }
  return DR_OK;
}

// Workspace, streams, the pilot decision (which reorders the pixels), and the uploads every batch reads.
int prepareRender(RenderPlan& P) {
  DrScene* sc = P.sc;
  const DrRenderDesc* rd = P.rd;
  const int spp = P.spp;
  const auto tAlloc0 = std::chrono::steady_clock::now();
  const uint32_t capBefore = sc->ws.cap;
  int rc = allocWorkspace(sc, sc->ws, P.wsCap, P.wsSf, P.wsPix, rd->max_tail, !P.traits->deviceGenerated && P.needTail > 0 && !P.packedTail, P.maxStateWords);
  if (rc) return rc;
  if (dr_opt("DARTRAY_VERBOSE") && sc->ws.cap != capBefore) {
    (void)hipDeviceSynchronize();
    fprintf(stderr, "dartray_hip: path-state workspace for %u slots (%.1f GB) allocated in %.1f ms\n", sc->ws.cap,
            (double)sc->ws.tiles.n * 4.0e-9 + (double)sc->ws.cap * 20.0e-9,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tAlloc0).count());
  }
  rc = allocSideBuffers(P);
  if (rc) return rc;
  if (P.envStage) HIP_TRY(sc->ws.envQ.alloc(sc->ws.cap));
  P.tgrid = traceGrid();
  rc = ensureSpill(sc, sc->ws, P.tgrid);
  if (rc) return rc;
  // the camera rays (a tile = 64 samples of one pixel) through the wave-coherent kernel k_trace_pk (DARTRAY_COHERENT_CAMERA=0: k_trace & co.)
  P.coherentCamera = !dr_opt("DARTRAY_COHERENT_CAMERA").isZero() && !P.dlSpec && P.traits->pixelBound;  // (else: a tile's slots are samples of 64 pixels)
  // lazy sample generation (DARTRAY_LAZY_GEN=0: every block for every pixel up front): needs the device sampler's compact form, the keyed
  // per-(pixel, block) streams (a block that is left out disturbs no other) and k_trace_pk's marks of the camera rays that hit
  P.lazyGen = lazyGenFor(P);
  // a stage's any-hit launch beside its closest-hit launch, on a second stream (DARTRAY_OVERLAP_ANY=0: one after the other)
  P.overlapAny = !dr_opt("DARTRAY_OVERLAP_ANY").isZero() && !P.dlSpec;
  if (P.overlapAny && !sc->s3) HIP_TRY(hipStreamCreateWithFlags(&sc->s3, hipStreamNonBlocking));
  // Which traversal kernel?  k_trace (one node per step, f32 filter) is issue bound and wins while the hot part of the tree stays in
  // cache; the pair kernels (half the dependent fetches) win on big incoherent trees (C4 hairball +26 %) and lose on others of the same
  // size; random probe rays mispredict both.  So the first big render of a big scene measures it ON ITS OWN WORK: small calibration
  // batches -- 64-pixel groups spread over the image -- are rendered first, into the film like every other batch: one with k_trace to
  // warm the caches, then one per candidate, timed; each ray kind keeps the kernel with the better time per algorithmic byte (the
  // device's own node / triangle counters of that batch).  Nothing is traced twice.  All kernels are bit-exact, so results do not depend
  // on the choice; dr_scene_set_trace_kernels / DARTRAY_TRACE_IMPL fix it (an N-rank host measures on rank 0 and hands the choice on).
  const DrOpt pilotOpt = dr_opt("DARTRAY_PILOT");  // 0: never; force: also on renders too small to need one (tests)
  const bool bigJob = (sc->d.nnodes >= (1u << 20) && (uint64_t)P.npixTotal * spp >= (1ull << 25)) || pilotOpt.is("force");
  const bool pilotOk = !pilotOpt.is("0") && P.traits->deviceGenerated && P.traits->pixelBound && !P.dlSpec && bigJob && P.npixTotal >= 3 * 64 * 4;
  P.calibrateTrace = !sc->traceCalibrated && pilotOk && !dr_opt("DARTRAY_TRACE_IMPL") && sc->d.pairs && !sc->d.nquads;
  P.measureLayout = !P.layoutKnown && pilotOk;
  if (P.measureLayout) P.L = &kLayout64;  // the batch whose stage lists are measured runs in the 64-slot layout
  P.pilotSets = P.calibrateTrace ? 4 : 1;
  P.calibPix = 0;
  if (P.calibrate()) {
    // (at least 2^24 samples per calibration batch: with 2^22 the launches are so short that their tails decide -- the pair kernel,
    // whose rays are half as many fetches long, looked 10 % faster than k_trace<0> on C2 and is 12 % slower at full size)
    uint64_t pilotSamples = std::min<uint64_t>(1ull << 25, std::max<uint64_t>(1ull << 24, (uint64_t)P.npixTotal * spp / 16));
    pilotSamples = std::min<uint64_t>(pilotSamples, (uint64_t)(P.pixPerBatch / 64 * 64) * spp);
    const size_t totalGroups = P.npixTotal / 64;
    const size_t groups = std::min<size_t>(std::max<size_t>(1, (size_t)(pilotSamples / spp) / 64), totalGroups / 4);
    P.calibPix = groups * 64;
    std::vector<int2> ordered;
    ordered.reserve(P.npixTotal);
    std::vector<uint8_t> taken(totalGroups, 0);
    for (int set = 0; set < P.pilotSets; ++set)
      for (size_t g = 0; g < groups; ++g) {
        const size_t grp = (((size_t)P.pilotSets * g + set) * totalGroups) / ((size_t)P.pilotSets * groups);  // interleaved: the sets see the same regions
        taken[grp] = 1;
        ordered.insert(ordered.end(), P.pixels.begin() + grp * 64, P.pixels.begin() + grp * 64 + 64);
      }
    for (size_t grp = 0; grp < totalGroups; ++grp)
      if (!taken[grp]) ordered.insert(ordered.end(), P.pixels.begin() + grp * 64, P.pixels.begin() + grp * 64 + 64);
    ordered.insert(ordered.end(), P.pixels.begin() + totalGroups * 64, P.pixels.end());
    P.pixels.swap(ordered);
  }
  if (!P.traits->pixelBound) {  // the pixel array is a batch's: k_gen_halton writes every slot's anchor pixel
    HIP_TRY(sc->ws.pix.alloc(P.cap));
    HIP_TRY(sc->ws.halton.alloc(P.cap));
  } else {
    HIP_TRY(sc->ws.pix.alloc(P.npixTotal));
    HIP_TRY(hipMemcpyAsync(sc->ws.pix.p, P.pixels.data(), P.npixTotal * sizeof(int2), hipMemcpyHostToDevice, P.s));
  }
  if (P.sampler == SamplerKind::Adaptive) {  // the list of flagged pixels: every pixel of the render at most
    HIP_TRY(sc->ws.adaptList.alloc(P.npixTotal));
    HIP_TRY(sc->ws.adaptCount.alloc(2));
    HIP_TRY(hipMemsetAsync(sc->ws.adaptCount.p, 0, 2 * sizeof(uint32_t), P.s));
  }
  HIP_TRY(hipMemcpyAsync(sc->ws.filterTable.p, rd->film.filter_table, 256 * sizeof(float), hipMemcpyHostToDevice, P.s));
  HIP_TRY(hipStreamSynchronize(P.s));  // (the copies read host memory the caller and this plan own)
  return DR_OK;
}

// What the two sample dumps share.  The plan of a render of these pixels / indices -- the same sample form, batches and launches -- its workspace,
// and the staging rows of a batch, [P.cap][stride] floats, zeroed (the words of a row behind the vector stay zero).
int prepareDump(RenderPlan& P, DevBuf<float>& aos, int stride) {
  int rc = planBatches(P);
  if (!rc) rc = allocWorkspace(P.sc, P.sc->ws, P.cap, P.sf, P.pixPerBatch, P.rd->max_tail, false, P.maxStateWords);
  if (rc) return rc;
  HIP_TRY(aos.alloc((size_t)P.cap * stride));
  HIP_TRY(hipMemsetAsync(aos.p, 0, (size_t)P.cap * stride * sizeof(float), P.s));
  return DR_OK;
}

// One batch's vectors to the caller: the sampler's launches for np entries of pix (nslots slots), the export, the copy to out.  The caller waits for the stream.
int dumpBatch(const RenderPlan& P, const int2* pix, uint32_t np, uint32_t nslots, float* aos, int stride, float* out) {
  const BatchState st = makeState(P.sc->ws, P.sf, pix, nslots, false, P.L->stateWords);
  P.genSamples(P.rp, st, np);
  P.L->export_samples(P.rp, st, aos, stride, P.s);
  HIP_TRY(hipGetLastError());  // (a launch that could not start)
  HIP_TRY(hipMemcpyAsync(out, aos, (size_t)nslots * stride * sizeof(float), hipMemcpyDeviceToHost, P.s));
  return DR_OK;
}

// dr_scene_last_render_info's word 3: -1 (rounds 4-5 reported the treelet-parked traversal's parking rounds here), or the integrator and
// the shading kernels of its own that ran -- bit 8: k_shade_whitted, bit 9: k_shade_spec
int32_t lastInfoWord(const RenderPlan& P) {
  switch (P.integrator) {  // (no default: -Wall names a kind this forgets)
    case IntegratorKind::DirectAll: case IntegratorKind::Path: case IntegratorKind::DirectOne: break;
    case IntegratorKind::Whitted: return DR_INTEGRATOR_WHITTED | 0x100 | (P.dlSpec ? 0x200 : 0);
    case IntegratorKind::AmbientOcclusion: return DR_INTEGRATOR_AO | 0x400;  // bit 10: k_shade_ao
    case IntegratorKind::Feature: return DR_INTEGRATOR_FEATURE | 0x800 | (P.feature.channel << 12);  // bit 11: k_shade_feature; bits 12-14: its channel
    case IntegratorKind::DiffusePRT: return DR_INTEGRATOR_DIFFUSE_PRT | 0x8000;  // bit 15: k_shade_prt
    case IntegratorKind::GlossyPRT: return DR_INTEGRATOR_GLOSSY_PRT | 0x10000;  // bit 16: k_shade_gprt + k_gprt_finish
    case IntegratorKind::UseProbes: return DR_INTEGRATOR_USE_PROBES | 0x20000;  // bit 17: k_shade_probes
    case IntegratorKind::Material: return DR_INTEGRATOR_MATERIAL | 0x40000 | (P.material.channel << 19);  // bit 18: k_shade_material; bit 19: its channel
  }
  return -1;
}

// dr_render_device, and dr_render_guides_device (g set, checked by the caller: the films of its channels in guideFilms).
int renderDevice(DrScene* sc, const DrRenderDesc* rd, void* film_dev, const DrGuidesDesc* g, void* const* guideFilms, void* hip_stream) {
  RenderPlan P;
  P.sc = sc;
  P.rd = rd;
  P.film = (float*)film_dev;
  P.s = (hipStream_t)hip_stream;
  int rc = planRender(P);
  if (rc) return rc;
  if (g) {
    P.guides.n = g->count;
    for (int i = 0; i < g->count; ++i) P.guides.mask |= 1u << g->channels[i];
    for (int i = 0; i < g->count; ++i) {
      P.guides.film[i] = (float*)guideFilms[i];
      P.guides.plane[i] = __builtin_popcount(P.guides.mask & ((1u << g->channels[i]) - 1u));  // (planes in DR_FEATURE_* order: k_guides)
    }
  }
  // recycle the events of earlier renders once they have completed (or when too many are pending)
  if (sc->lastEvent && !sc->traceEvents.empty()) {
    hipError_t q = hipEventQuery(sc->lastEvent);
    if (q != hipSuccess && sc->eventsUsed > 8192) q = hipEventSynchronize(sc->lastEvent);
    if (q == hipSuccess) sc->foldEvents();
    (void)hipGetLastError();  // hipErrorNotReady is not an error
  }
  sc->adaptiveN = 0;
  sc->statsPending = true;
  hipEvent_t evStart = sc->getEvent(), evStop = sc->getEvent();
  sc->renderEvents.push_back({evStart, evStop});
  sc->lastEvent = evStop;
  HIP_TRY(hipEventRecord(evStart, P.s));
  if (P.npixTotal == 0) {
    HIP_TRY(hipEventRecord(evStop, P.s));
    return DR_OK;
  }
  rc = planBatches(P);
  if (rc) return rc;
  rc = prepareRender(P);
  if (rc) return rc;
  PilotResult pilot;
  if (P.calibrate()) {
    rc = runPilot(P, pilot);
    if (rc) return rc;
  }
  uint64_t cameraSamples = (uint64_t)P.npixTotal * P.spp, nBatches = P.nBatches;
  if (P.sampler == SamplerKind::Halton) {  // one host wait per batch: how many indices of its range the window accepted
    rc = runHaltonBatches(P, &cameraSamples);
  } else {  // (a calibration set that was skipped left its pixels to the ordinary batches)
    rc = runBatches(P, sc->ws.pix.p, (size_t)pilot.setsRun * P.calibPix);
  }
  if (rc) return rc;
  bool lazy2 = false;
  if (P.sampler == SamplerKind::Adaptive) {
    // the one host round trip of the mode: how many pixels the first pass flagged (and how many of them the film holds)
    uint32_t counts[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(counts, sc->ws.adaptCount.p, sizeof(counts), hipMemcpyDeviceToHost, P.s));
    HIP_TRY(hipStreamSynchronize(P.s));
    const uint32_t nFlagged = (uint32_t)std::min<uint64_t>(counts[0], P.npixTotal);
    sc->adaptiveN = nFlagged;
    if (nFlagged) {
      std::vector<int2>().swap(P.pixels);  // (uploaded; the second plan need not copy them)
      RenderPlan Q = secondPass(P, nFlagged);
      rc = runBatches(Q, sc->ws.adaptList.p, 0);
      if (rc) return rc;
      cameraSamples += (uint64_t)nFlagged * Q.spp;
      P.filmSamples += (uint64_t)counts[1] * (uint64_t)(Q.spp - P.spp);  // (their first-pass samples were not added)
      nBatches += Q.nBatches;
      lazy2 = Q.lazyGen;
    }
  }
  HIP_TRY(hipEventRecord(evStop, P.s));
  sc->stats.camera_samples += cameraSamples;
  sc->stats.film_samples += P.filmSamples;
  if (cameraSamples >= (1ull << 25)) sc->bigRenders++;  // (planBatches: the next render of this scene may take the whole image as one batch)
  sc->lastInfo[0] = P.L == &kLayoutSp4 ? 4 : 64;
  sc->lastInfo[1] = P.L->trace_kernel_id(sc->d, 0);
  sc->lastInfo[2] = P.L->trace_kernel_id(sc->d, 1);
  sc->lastInfo[3] = lastInfoWord(P);
  sc->lastInfo[4] = pilot.setsRun;
  sc->lastInfo[5] = (int32_t)std::min<uint64_t>(0x7fffffff, nBatches);
  sc->lastInfo[6] = P.tgrid / std::max(1, g_numCU);
  sc->lastInfo[7] = (P.overlapAny ? 1 : 0) | (P.coherentCamera && !sc->d.nquads ? 2 : 0) | (P.lazyGen || lazy2 ? 8 : 0);
  return DR_OK;
}

}  // namespace

extern "C" {

int dr_render_device(DrScene* sc, const DrRenderDesc* rd, void* film_dev, void* hip_stream) {
  if (!sc || !rd || !film_dev) return fail(DR_ERR_INVALID, "null argument");
  return renderDevice(sc, rd, film_dev, nullptr, nullptr, hip_stream);
}

int dr_render_guides_device(DrScene* sc, const DrRenderDesc* rd, const DrGuidesDesc* g, void* film_dev, void* const* guide_films_dev, void* hip_stream) {
  if (!sc || !rd || !g || !film_dev || !guide_films_dev) return fail(DR_ERR_INVALID, "null argument");
  int rc = dr_render_guides_check(rd, g, sc->d.ntris);
  if (rc) return rc;
  for (int i = 0; i < g->count; ++i)
    if (!guide_films_dev[i]) return fail(DR_ERR_INVALID, "render guides: a channel's film is null");
  return renderDevice(sc, rd, film_dev, g, guide_films_dev, hip_stream);
}

int dr_enumerate_pixels(const DrRenderDesc* rd, int32_t* out_xy, uint64_t cap, uint64_t* n_out) {
  if (!rd || !n_out) return fail(DR_ERR_INVALID, "null argument");
  RenderParams rp;
  memset(&rp, 0, sizeof(rp));
  rp_film(rp, rd->film);
  std::vector<int2> pixels;
  enumeratePixels(rp, rd, pixels);
  *n_out = pixels.size();
  if (out_xy) {
    if (cap < pixels.size()) return fail(DR_ERR_INVALID, "pixel buffer too small");
    for (size_t i = 0; i < pixels.size(); ++i) {
      out_xy[2 * i] = pixels[i].x;
      out_xy[2 * i + 1] = pixels[i].y;
    }
  }
  return DR_OK;
}

int dr_scene_get_adaptive_pixels(DrScene* sc, int32_t* out_xy, uint64_t cap, uint64_t* n_out) {
  if (!sc || !n_out) return fail(DR_ERR_INVALID, "null argument");
  *n_out = sc->adaptiveN;
  if (out_xy && sc->adaptiveN) {
    if (cap < sc->adaptiveN) return fail(DR_ERR_INVALID, "pixel buffer too small");
    // (the render waited for the list's length before it started the second pass: the list is complete)
    HIP_TRY(hipMemcpy(out_xy, sc->ws.adaptList.p, (size_t)sc->adaptiveN * sizeof(int2), hipMemcpyDeviceToHost));
  }
  return DR_OK;
}

int dr_generate_samples(DrScene* sc, const DrRenderDesc* rd, const int32_t* pixel_xy, uint64_t npix, float* out, int32_t stride) {
  if (!sc || !rd || !pixel_xy || !out) return fail(DR_ERR_INVALID, "null argument");
  if (rd->sampler_mode == DR_SAMPLER_HOST_BUFFER) return fail(DR_ERR_INVALID, "dr_generate_samples: the host-buffer mode has no device sampler");
  if (rd->sampler_mode == DR_SAMPLER_HALTON) return fail(DR_ERR_INVALID, "dr_generate_samples: the halton sampler's samples are not bound to pixels (dr_generate_halton_samples takes a range of the sequence)");
  if (npix == 0) return DR_OK;
  RenderPlan P;
  P.sc = sc;
  P.rd = rd;
  int rc = planRender(P);
  if (rc) return rc;
  if (stride < P.rp.nFloats) return fail(DR_ERR_INVALID, "dr_generate_samples: stride smaller than the sample vector");
  if (npix * (uint64_t)P.spp >= (1ull << 31)) return fail(DR_ERR_UNSUPPORTED, "dr_generate_samples: more than 2^31 samples in one call");
  P.rp.genMask = 0ull;  // (every LD block produced)
  P.pixels.resize(npix);
  for (uint64_t i = 0; i < npix; ++i) P.pixels[i] = make_int2(pixel_xy[2 * i], pixel_xy[2 * i + 1]);
  P.npixTotal = P.pixels.size();
  DevBuf<float> aos;
  rc = prepareDump(P, aos, stride);
  if (rc) return rc;
  HIP_TRY(sc->ws.pix.alloc(P.npixTotal));
  HIP_TRY(hipMemcpyAsync(sc->ws.pix.p, P.pixels.data(), P.npixTotal * sizeof(int2), hipMemcpyHostToDevice, P.s));
  for (size_t p0 = 0; p0 < P.npixTotal; p0 += P.pixPerBatch) {
    const uint32_t np = (uint32_t)std::min<size_t>(P.pixPerBatch, P.npixTotal - p0);
    rc = dumpBatch(P, sc->ws.pix.p + p0, np, np * (uint32_t)P.spp, aos.p, stride, out + p0 * P.spp * (size_t)stride);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(P.s));
  }
  return DR_OK;
}

int dr_generate_halton_samples(DrScene* sc, const DrRenderDesc* rd, uint64_t first_index, uint64_t count, uint64_t* k_out, int32_t* pixel_xy_out,
                               float* out, int32_t stride, uint64_t* n_out) {
  if (!sc || !rd || !n_out) return fail(DR_ERR_INVALID, "null argument");
  *n_out = 0;
  if (rd->sampler_mode != DR_SAMPLER_HALTON) return fail(DR_ERR_INVALID, "dr_generate_halton_samples: sampler_mode must be DR_SAMPLER_HALTON");
  RenderPlan P;
  P.sc = sc;
  P.rd = rd;
  int rc = planRender(P);
  if (rc) return rc;
  if (first_index > P.npixTotal || count > P.npixTotal - first_index)
    return fail(DR_ERR_INVALID, "dr_generate_halton_samples: the range leaves the task's sequence (pixelsamples * max(width, height)^2 indices)");
  if (count == 0) return DR_OK;
  if (!k_out || !pixel_xy_out || !out) return fail(DR_ERR_INVALID, "null argument");
  if (stride < P.rp.nFloats) return fail(DR_ERR_INVALID, "dr_generate_halton_samples: stride smaller than the sample vector");
  P.npixTotal = (size_t)count;
  DevBuf<float> aos;
  rc = prepareDump(P, aos, stride);
  if (rc) return rc;
  Workspace& w = sc->ws;
  HIP_TRY(w.pix.alloc(P.cap));
  HIP_TRY(w.halton.alloc(P.cap));
  uint64_t done = 0;
  for (uint64_t i0 = 0; i0 < count; i0 += P.pixPerBatch) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(P.pixPerBatch, count - i0);
    uint32_t accepted = 0;
    rc = haltonSelect(P, first_index + i0, n, &accepted);
    if (rc) return rc;
    if (accepted > n) return fail(DR_ERR_HIP, "halton sampler: the selection accepted more indices than its range holds");
    if (accepted == 0) continue;
    rc = dumpBatch(P, w.pix.p, accepted, accepted, aos.p, stride, out + done * (size_t)stride);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(k_out + done, w.halton.idx.p, (size_t)accepted * sizeof(uint64_t), hipMemcpyDeviceToHost, P.s));
    HIP_TRY(hipMemcpyAsync(pixel_xy_out + 2 * done, w.pix.p, (size_t)accepted * sizeof(int2), hipMemcpyDeviceToHost, P.s));
    HIP_TRY(hipStreamSynchronize(P.s));
    done += accepted;
  }
  *n_out = done;
  return DR_OK;
}

int dr_get_stats(DrScene* sc, DrRenderStats* out) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  if (sc->statsPending) {
    if (sc->lastEvent) HIP_TRY(hipEventSynchronize(sc->lastEvent));
    TraceCounters c;
    HIP_TRY(hipMemcpy(&c, sc->ctr.p, sizeof(c), hipMemcpyDeviceToHost));
    sc->stats.closest_rays = c.closest_rays; sc->stats.any_rays = c.any_rays;
    sc->stats.closest_nodes = c.closest_nodes; sc->stats.any_nodes = c.any_nodes;
    sc->stats.closest_tris = c.closest_tris; sc->stats.any_tris = c.any_tris;
    sc->stats.shade_items = c.shade_items; sc->stats.shade_vertices = c.shade_vertices;
    sc->stats.shade_cont = c.shade_cont; sc->stats.shade_mis = c.shade_mis; sc->stats.shade_shadow = c.shade_shadow;
    sc->pkRays = c.pk_rays[0];
    sc->pkNodes = c.pk_nodes[0];
    sc->pkTris = c.pk_tris[0];
    sc->genDone = sc->genDoneHost + c.gen_pixel_blocks;
    sc->foldEvents();
    sc->statsPending = false;
    shade_prof_dump();
    trace_prof_dump();
    sp4::shade_prof_dump();
    sp4::trace_prof_dump();
  }
  *out = sc->stats;
  return DR_OK;
}

int dr_reset_stats(DrScene* sc) {
  if (!sc) return fail(DR_ERR_INVALID, "null argument");
  if (sc->lastEvent) HIP_TRY(hipEventSynchronize(sc->lastEvent));
  memset(&sc->stats, 0, sizeof(sc->stats));
  sc->traceEvents.clear();
  sc->renderEvents.clear();
  sc->eventsUsed = 0;
  sc->lastEvent = nullptr;
  sc->statsPending = false;
  sc->pkMs = 0.0;
  sc->pkLaunches = 0;
  sc->pkRays = sc->pkNodes = sc->pkTris = 0;
  sc->genDone = sc->genDoneHost = sc->genNamed = 0;
  HIP_TRY(hipMemset(sc->ctr.p, 0, sizeof(TraceCounters)));
  return DR_OK;
}

int dr_scene_get_sampler_stats(DrScene* sc, double out[2]) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  DrRenderStats st;
  const int rc = dr_get_stats(sc, &st);
  if (rc) return rc;
  out[0] = (double)sc->genDone;
  out[1] = (double)sc->genNamed;
  return DR_OK;
}

int dr_scene_get_coherent_stats(DrScene* sc, double out[5]) {
  if (!sc || !out) return fail(DR_ERR_INVALID, "null argument");
  DrRenderStats st;
  const int rc = dr_get_stats(sc, &st);  // (waits for the renders in flight and folds their events, like dr_get_stats)
  if (rc) return rc;
  out[0] = (double)sc->pkRays;
  out[1] = (double)sc->pkNodes;
  out[2] = (double)sc->pkTris;
  out[3] = (double)sc->pkLaunches;
  out[4] = sc->pkMs;
  return DR_OK;
}

int dr_film_resolve_device(const void* film_dev, int64_t npixels, void* rgb_dev, void* hip_stream) {
  if (!film_dev || !rgb_dev || npixels < 0) return fail(DR_ERR_INVALID, "null argument");
  if (npixels == 0) return DR_OK;
  launch_film_resolve((const float*)film_dev, npixels, (float*)rgb_dev, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return DR_OK;
}

int dr_render(DrScene* sc, const DrRenderDesc* rd, float* film_out, float* rgb_out) {
  if (!sc || !rd || !film_out) return fail(DR_ERR_INVALID, "null argument");
  RenderParams rp;
  memset(&rp, 0, sizeof(rp));
  rp_film(rp, rd->film);
  const int64_t npix = (int64_t)rp.width * rp.height;
  DevBuf<float> film, rgb;
  HIP_TRY(film.alloc(4 * npix));
  HIP_TRY(hipMemset(film.p, 0, 4 * npix * sizeof(float)));
  int rc = dr_render_device(sc, rd, film.p, nullptr);
  if (rc) return rc;
  if (rgb_out) {
    HIP_TRY(rgb.alloc(3 * npix));
    rc = dr_film_resolve_device(film.p, npix, rgb.p, nullptr);
    if (rc) return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(film_out, film.p, 4 * npix * sizeof(float), hipMemcpyDeviceToHost));
  if (rgb_out) HIP_TRY(hipMemcpy(rgb_out, rgb.p, 3 * npix * sizeof(float), hipMemcpyDeviceToHost));
  return DR_OK;
}

int dr_render_guides(DrScene* sc, const DrRenderDesc* rd, const DrGuidesDesc* g, float* film_out, float* rgb_out, float* const* guide_films_out,
                     float* const* guide_rgbs_out) {
  if (!sc || !rd || !g || !film_out || !guide_films_out) return fail(DR_ERR_INVALID, "null argument");
  int rc = dr_render_guides_check(rd, g, sc->d.ntris);
  if (rc) return rc;
  for (int i = 0; i < g->count; ++i)
    if (!guide_films_out[i]) return fail(DR_ERR_INVALID, "render guides: a channel's film is null");
  RenderParams rp;
  memset(&rp, 0, sizeof(rp));
  rp_film(rp, rd->film);
  const int64_t npix = (int64_t)rp.width * rp.height;
  // the beauty film, then the channels' films, one after the other in one buffer; one more image to resolve into
  const int n = g->count;
  DevBuf<float> films, rgb;
  HIP_TRY(films.alloc((size_t)(n + 1) * 4 * npix));
  HIP_TRY(hipMemset(films.p, 0, (size_t)(n + 1) * 4 * npix * sizeof(float)));
  void* guideDev[DR_GUIDES_MAX] = {};
  for (int i = 0; i < n; ++i) guideDev[i] = films.p + (size_t)(i + 1) * 4 * npix;
  rc = dr_render_guides_device(sc, rd, g, films.p, guideDev, nullptr);
  if (rc) return rc;
  HIP_TRY(rgb.alloc(3 * npix));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(film_out, films.p, 4 * npix * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) HIP_TRY(hipMemcpy(guide_films_out[i], guideDev[i], 4 * npix * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = -1; i < n; ++i) {  // (-1: the beauty image)
    float* out = i < 0 ? rgb_out : (guide_rgbs_out ? guide_rgbs_out[i] : nullptr);
    if (!out) continue;
    rc = dr_film_resolve_device(i < 0 ? (void*)films.p : guideDev[i], npix, rgb.p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, rgb.p, 3 * npix * sizeof(float), hipMemcpyDeviceToHost));
  }
  return DR_OK;
}

int dr_render_sharded(DrScene* sc, const DrRenderDesc* rd, int32_t root, float* film_out, float* rgb_out) {
  if (!sc || !rd) return fail(DR_ERR_INVALID, "null argument");
  const int world = dr_comm_world(), rank = dr_comm_rank();
  if (world > 1 ? (root < 0 || root >= world) : root != 0) return fail(DR_ERR_INVALID, "dr_render_sharded: root out of range");
  RenderParams rp;
  memset(&rp, 0, sizeof(rp));
  rp_film(rp, rd->film);
  const int64_t npix = (int64_t)rp.width * rp.height;
  DevBuf<float> film, rgb;
  HIP_TRY(film.alloc(4 * npix));
  HIP_TRY(hipMemset(film.p, 0, 4 * npix * sizeof(float)));
  int rc = dr_render_device(sc, rd, film.p, nullptr);
  if (rc) return rc;
  if (world > 1) {
    rc = dr_film_reduce(film.p, npix, root, nullptr);
    if (rc) return rc;
  }
  const bool isRoot = world > 1 ? rank == root : true;
  if (isRoot && rgb_out) {
    HIP_TRY(rgb.alloc(3 * npix));
    rc = dr_film_resolve_device(film.p, npix, rgb.p, nullptr);
    if (rc) return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (isRoot && film_out) HIP_TRY(hipMemcpy(film_out, film.p, 4 * npix * sizeof(float), hipMemcpyDeviceToHost));
  if (isRoot && rgb_out) HIP_TRY(hipMemcpy(rgb_out, rgb.p, 3 * npix * sizeof(float), hipMemcpyDeviceToHost));
  return DR_OK;
}

int dr_copy_bandwidth(uint64_t bytes, int32_t iters, double* gbps_out) {
  if (g_device < 0) return fail(DR_ERR_NO_DEVICE, "dr_init has not been called");
  if (!gbps_out || bytes < 16 || iters <= 0) return fail(DR_ERR_INVALID, "bad argument");
  uint64_t n4 = bytes / 16;
  DevBuf<float4> a, b;
  HIP_TRY(a.alloc(n4));
  HIP_TRY(b.alloc(n4));
  HIP_TRY(hipMemset(a.p, 1, n4 * 16));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  launch_copy(a.p, b.p, n4, 0);
  HIP_TRY(hipEventRecord(e0, 0));
  for (int i = 0; i < iters; ++i) launch_copy(a.p, b.p, n4, 0);
  HIP_TRY(hipEventRecord(e1, 0));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *gbps_out = (2.0 * (double)n4 * 16.0 * iters) / ((double)ms * 1.0e-3) / 1.0e9;
  return DR_OK;
}

}  // extern "C"
