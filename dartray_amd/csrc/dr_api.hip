// dr_api.hip -- the C ABI of include/dartray_hip.h: options, the render planner, film, statistics and every entry point but
// dr_scene_create / dr_scene_destroy (dr_scene_build.hip).  The batches a render plans run in dr_batch.hip; dr_host.h is what
// the three share.
//
// Host logic restated from the reference where it decides WHAT is traced:
//   sampler window       ImageFilm.getSampleExtent (film/image_film.dart:247-252),
//                        GetSubWindow (core/common.dart:52-73), dartray.dart:1009-1023
//   pixel order          LinearPixelSampler (pixel_samplers/linear_pixel_sampler.dart:29-40)
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
int g_numCU = 256;
#define DR_STATE_WORDS F_SAMPLES  // 41 4-byte words of fixed path state per slot: 3 f64 + 10 3-vectors + 5 i32

}  // namespace

namespace dr_host {

int g_device = -1;

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
// dr_render_device, in units: RenderPlan (dr_host.h; what this call runs: planRender, planBatches -- here), prepareRender
// (workspace, pilot decision, uploads -- here), BatchRunner (one batch through the stage loop), runBatches and runPilot (the
// calibration batches) -- dr_batch.hip -- and the entry point, here, which strings them together and records what ran.
// ===========================================================================
namespace {

// What the call asks for, checked, as RenderParams + the facts every later unit reads; which pixels it traces.  Callable without a film (the two
// sample dumps plan this way).  Every check runs where it always ran, so that of two broken rules the same one wins.
int planRender(RenderPlan& P) {
  DrScene* sc = P.sc;
  const DrRenderDesc* rd = P.rd;
  // ---- the sampler mode: its kind, its own rules, the samples per pixel of this plan ----
  static const SamplerKind kinds[] = {SamplerKind::HostBuffer, SamplerKind::LowDiscrepancy, SamplerKind::Stratified, SamplerKind::Stratified, SamplerKind::Adaptive, SamplerKind::Halton, SamplerKind::Random};
  static_assert(DR_SAMPLER_HOST_BUFFER == 0 && DR_SAMPLER_COUNTER == 1 && DR_SAMPLER_STRATIFIED == 2 && DR_SAMPLER_STRATIFIED_NOJITTER == 3 && DR_SAMPLER_ADAPTIVE == 4 && DR_SAMPLER_HALTON == 5 && DR_SAMPLER_RANDOM == 6, "kinds[] is indexed by sampler_mode");
  const bool knownMode = rd->sampler_mode >= 0 && rd->sampler_mode <= DR_SAMPLER_RANDOM;
  P.sampler = knownMode ? kinds[rd->sampler_mode] : SamplerKind::LowDiscrepancy;  // (an unknown mode is refused where the pixel source is chosen, as ever)
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
  // ---- the integrator, the camera and the film into rp; the state layout; the stages ----
  if (!knownIntegrator(rd->integrator)) return fail(DR_ERR_INVALID, "unknown integrator");
  P.integrator = (IntegratorKind)rd->integrator;  // (kIntegratorTraits' static_assert: the kinds are the ABI's values)
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
  // the stages: where a stage's DirectStage entry comes from, and how many stages a round of the stage loop runs
  rp.dstages = sc->dlStages.p;
  rp.nDirectStages = 0;
  switch (P.integrator) {  // (no default: -Wall names a kind this forgets)
    case IntegratorKind::DirectAll: rp.nDirectStages = sc->dlNStages; P.nStages = rp.nDirectStages + 1; break;  // the scene's table from its start
    case IntegratorKind::DirectOne:  // strategy "one": the last entry of the scene's stage table, an arithmetic slot layout
      rp.dstages += sc->dlNStages;
      rp.nDirectStages = sc->d.nlights ? 1 : 0;
      P.nStages = rp.nDirectStages + 1;
      break;
    case IntegratorKind::Path: P.nStages = rd->max_depth + 2; break;
    case IntegratorKind::Whitted: P.nStages = rp.nLights + 1; break;  // one per light
    case IntegratorKind::AmbientOcclusion: {
      // AmbientOcclusionIntegrator (ambient_occlusion_integrator.dart:24-26,55-60): nSamples = RoundUpPow2(ns) occlusion rays per camera
      // hit, one per stage.  A render holds at most CounterLayout::maxStages() stages, so the rays go in rounds of the stage loop, 128 to a round
      // (a power of two: it divides every larger nSamples); a round is one stage more than its rays, since the last ray is folded in by a stage
      // that queues nothing.
      if (rd->ao_nsamples < 1) return fail(DR_ERR_INVALID, "ambient occlusion integrator: nsamples must be at least 1");
      uint32_t ns = 1;
      while (ns < (uint32_t)rd->ao_nsamples) ns <<= 1;  // RoundUpPow2 (common.dart:117-125)
      if (ns > 4096) return fail(DR_ERR_INVALID, "ambient occlusion integrator: nsamples above 4096 after rounding up to a power of two (the samplers' cap)");
      if (!(rd->ao_mindist >= 0.0)) return fail(DR_ERR_INVALID, "ambient occlusion integrator: mindist must not be negative");
      if (!(rd->ao_maxdist > rd->ao_mindist)) return fail(DR_ERR_INVALID, "ambient occlusion integrator: maxdist must be greater than mindist");
      P.ao.nSamples = (int)ns;
      P.ao.perRound = std::min(P.ao.nSamples, 128);
      P.ao.rounds = P.ao.nSamples / P.ao.perRound;
      P.ao.minDist = rd->ao_mindist;
      P.ao.maxDist = rd->ao_maxdist;
      P.nStages = P.ao.perRound + 1;
      break;
    }
    case IntegratorKind::Feature: {  // the camera hit itself, one stage, nothing traced behind it
      int code = DR_OK;
      if (const char* why = featureRefusal(rd->feature_channel, sc->d.ntris, &code)) return fail(code, why);
      P.feature.channel = rd->feature_channel;
      P.nStages = 1;
      break;
    }
    case IntegratorKind::DiffusePRT: {
      // DiffusePRTIntegrator (diffuse_prt_integrator.dart:24-31,83-87): nSamples = RoundUpPow2(ns) occlusion rays per camera hit, one
      // per stage, in ambient occlusion's rounds of 128.  Materials other than a Lambertian matte are refused by name: rho2's 36-sample estimate
      // of their lobes has no device function outside the kernels that own them.
      if (const char* why = prtRefusal(rd->prt_lmax, rd->prt_nsamples, true)) return fail(DR_ERR_INVALID, why);
      static const char* const names[] = {"matte with sigma != 0 (Oren-Nayar)", "matte", "mirror", "glass", "plastic"};
      for (size_t i = 0; i < sc->prtMaterials.size(); ++i)
        if (sc->prtMaterials[i] != DR_MATERIAL_MATTE)
          return fail(DR_ERR_UNSUPPORTED, std::string("diffuse PRT: material ") + names[std::min(3, std::max(-1, sc->prtMaterials[i])) + 1] + " (material " +
                                              std::to_string(i) + " of the scene) is not supported: only matte with sigma 0 is");
      uint32_t ns = 1;
      while (ns < (uint32_t)rd->prt_nsamples) ns <<= 1;  // RoundUpPow2 (common.dart:117-125)
      P.prt.nSamples = (int)ns;
      P.prt.perRound = std::min(P.prt.nSamples, 128);
      P.prt.rounds = P.prt.nSamples / P.prt.perRound;
      P.prt.lmax = rd->prt_lmax;
      P.nStages = P.prt.perRound + 1;
      break;
    }
    case IntegratorKind::GlossyPRT: {
      // GlossyPRTIntegrator (glossy_prt_integrator.dart:24-25,118-125): DiffusePRT's rays, stages and rounds -- every ray is traced --
      // and no material function is read, so no material is refused
      if (const char* why = gprtRefusal(rd->prt_lmax, rd->prt_nsamples, true)) return fail(DR_ERR_INVALID, why);
      uint32_t ns = 1;
      while (ns < (uint32_t)rd->prt_nsamples) ns <<= 1;  // RoundUpPow2 (common.dart:117-125)
      P.gprt.nSamples = (int)ns;
      P.gprt.perRound = std::min(P.gprt.nSamples, 128);
      P.gprt.rounds = P.gprt.nSamples / P.gprt.perRound;
      P.gprt.lmax = rd->prt_lmax;
      P.gprt.words = std::max(1, P.gprt.nSamples / 32);
      P.nStages = P.gprt.perRound + 1;
      break;
    }
    case IntegratorKind::UseProbes: {
      // UseProbesIntegrator (use_probes_integrator.dart:90-162): the camera hit and the scene's probe grid, one stage, nothing traced
      // behind it.  rho2 of anything but a Lambertian matte has no device function outside the kernels that own it: refused by name, as under diffuse PRT
      if (sc->probes.lmax == 0) return fail(DR_ERR_INVALID, "use probes: no probe grid is set on the scene (dr_scene_set_probes)");
      if (sc->probes.includeDirect == 0)
        return fail(DR_ERR_UNSUPPORTED, "use probes: a grid with includeDirect 0 is not supported (that path adds UniformSampleAllLights at every hit); bake with directlighting true");
      static const char* const names[] = {"matte with sigma != 0 (Oren-Nayar)", "matte", "mirror", "glass", "plastic"};
      for (size_t i = 0; i < sc->prtMaterials.size(); ++i)
        if (sc->prtMaterials[i] != DR_MATERIAL_MATTE)
          return fail(DR_ERR_UNSUPPORTED, std::string("use probes: material ") + names[std::min(3, std::max(-1, sc->prtMaterials[i])) + 1] + " (material " +
                                              std::to_string(i) + " of the scene) is not supported: only matte with sigma 0 is");
      P.nStages = 1;
      break;
    }
    case IntegratorKind::Material: {  // the camera hit's material colour or emitted radiance, one stage, nothing traced behind it
      if (const char* why = materialRefusal(rd->material_channel)) return fail(DR_ERR_INVALID, why);
      P.material.channel = rd->material_channel;
      P.nStages = 1;
      break;
    }
  }
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
  // ---- the mode's rules that have always run behind the integrator's, max_depth's and the camera's refusals above (strat_xsamples reads only spp, but a descriptor
  // that also names an unknown integrator keeps that refusal); which pixels: the caller's list, the task's / tile share's, or -- not pixel bound -- a window ----
  if (P.sampler == SamplerKind::Stratified) {
    P.strat.x = rd->strat_xsamples;
    if (P.strat.x <= 0 || spp % P.strat.x != 0)
      return fail(DR_ERR_INVALID, "stratified sampler: strat_xsamples must be positive and divide spp (spp = xsamples * ysamples)");
  }
  // roundSize is the identity (stratified_sampler.dart:63-65, halton_sampler.dart:102-104, random_sampler.dart:90-92) while the scene's DirectLighting slot layout is
  // LowDiscrepancySampler's rounded one, so a light's nsamples must be its own rounding
  if (P.traits->identityRoundSize && P.integ->sceneSlots)
    for (int n : sc->lightNSamples)
      if (n > 1 && (n & (n - 1)) != 0) return fail(DR_ERR_UNSUPPORTED, P.traits->identityRoundSize);
  if (P.sampler == SamplerKind::Adaptive && rp.blocks && P.adaptive.max > 1024)
    return fail(DR_ERR_UNSUPPORTED, "adaptive sampler: maxSamples > 1024 with LD blocks of several entries per sample (DirectLighting with nsamples > 1): the float-form sampler's table exceeds the LDS");
  if (P.sampler == SamplerKind::HostBuffer) {
    if (rd->nsamples <= 0 || rd->nsamples % spp != 0 || !rd->pixel_xy || !rd->sample_vec)
      return fail(DR_ERR_INVALID, "host-buffer sampler: nsamples must be a positive multiple of spp with pixel_xy and sample_vec set");
    if (rd->sample_stride < rp.nFloats) return fail(DR_ERR_INVALID, "sample_stride smaller than the sample vector");
    if (P.needTail > 0 && (!rd->tail || rd->max_tail < P.needTail))
      return fail(DR_ERR_INVALID, "host-buffer sampler: tail buffer missing or max_tail too small for max_depth");
    P.packedTail = P.needTail > 0 && rd->tail_offsets != nullptr;  // (its device buffers are sized per batch: BatchRunner::loadSamples)
    if (P.packedTail && rd->tail_offsets[rd->nsamples] < rd->tail_offsets[0])
      return fail(DR_ERR_INVALID, "host-buffer sampler: tail_offsets must be non-decreasing");
    const int64_t np = rd->nsamples / spp;
    P.pixels.resize(np);
    for (int64_t i = 0; i < np; ++i) P.pixels[i] = make_int2(rd->pixel_xy[2 * i], rd->pixel_xy[2 * i + 1]);
  } else if (P.traits->pixelBound) {
    if (!knownMode) return fail(DR_ERR_INVALID, "unknown sampler mode");
    enumeratePixels(rp, rd, P.pixels);
  } else {
    // Halton: the task's window as the reference hands it to the sampler (GetSubWindow's extents as they are: see enumeratePixels)
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
  }
  if (P.traits->pixelBound) {
    P.npixTotal = P.pixels.size();
    P.filmSamples = 0;
    for (const int2& p : P.pixels)
      if (p.x >= rp.left && p.x < rp.left + rp.width && p.y >= rp.top && p.y < rp.top + rp.height) P.filmSamples += spp;
  }
  if (P.nStages > CounterLayout::maxStages()) return fail(DR_ERR_UNSUPPORTED, "too many stages");
  return DR_OK;
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
    // indices in the compact form, 4 B per float otherwise; + the RNG tail in host-buffer mode).  On a device with less free
    // memory the batch shrinks instead of failing (results do not depend on the batch size).
    const uint64_t tailPerSlot = !(!P.traits->deviceGenerated && P.needTail > 0) ? 0ull
                                 : (P.packedTail ? 16ull + 8ull * ((rd->tail_offsets[rd->nsamples] - rd->tail_offsets[0]) / (uint64_t)rd->nsamples + 1ull)
                                                 : (uint64_t)rd->max_tail * 8);
    const uint64_t perSlot = (uint64_t)P.maxStateWords * 4 + (uint64_t)(P.wsSf.svWords() + 15) / 16 + 20 + tailPerSlot + (!P.traits->deviceGenerated ? (uint64_t)rd->sample_stride * 4 : 0) +
                             (sf.compact ? (uint64_t)(16 * sf.nBlocks + spp - 1) / spp : 0) +  // scramble words + generator states, per (block, pixel)
                             (P.dlSpec ? (uint64_t)std::max(1, rd->max_depth) * sizeof(SpecFrame) + 12 : 0) +
                             (P.prt.lmax ? (uint64_t)sh_terms(P.prt.lmax) * 4 + 8 : 0) +  // diffuse PRT: the slot's transfer coefficients + the round lists
                             (P.gprt.lmax ? (uint64_t)P.gprt.words * 4 + 4 + 8 : 0) +  // glossy PRT: the slot's visibility words, its hit mark + the round lists
                             (uint64_t)P.guides.n * 12;  // a guide render: a side plane of three floats per channel
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
bool lazyGenFor(const RenderPlan& P);
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
  if (P.dlSpec) {
    HIP_TRY(sc->ws.specFrames.alloc((size_t)sc->ws.cap * std::max(1, rd->max_depth) * DR_SPEC_FRAME_WORDS));
    HIP_TRY(sc->ws.specSp.alloc(sc->ws.cap));
    HIP_TRY(sc->ws.roundA.alloc(sc->ws.cap));
    HIP_TRY(sc->ws.roundB.alloc(sc->ws.cap));
  }
  if (P.shadowRounds() > 1) {  // ambient occlusion / diffuse PRT in rounds: the slots that hit, handed from a round's last stage to the next round's first
    HIP_TRY(sc->ws.roundA.alloc(sc->ws.cap));
    HIP_TRY(sc->ws.roundB.alloc(sc->ws.cap));
  }
  if (P.integrator == IntegratorKind::DiffusePRT) {
    // the side buffer of transfer coefficients, [Terms(lmax)][wsCap] -- this plan's batch capacity, which planBatches shrank to fit, not the
    // capacity an earlier, larger render left the workspace with -- and, once per scene and lmax, before the first batch, the incident light
    HIP_TRY(sc->ws.prt.alloc((size_t)P.wsCap * (size_t)sh_terms(P.prt.lmax)));
    rc = prtIncident(sc, P.prt.lmax, rd->camera.shutter_open, P.s);
    if (rc) return rc;
  }
  if (P.integrator == IntegratorKind::GlossyPRT) {
    // the side buffers, sized like diffuse PRT's by this plan's batch capacity, and, once per scene and key, before the first batch, the incident
    // light and the BSDF matrix (ComputeBSDFMatrix(..., 1024, lmax): glossy_prt_integrator.dart:48)
    HIP_TRY(sc->ws.gprtBits.alloc((size_t)P.wsCap * (size_t)P.gprt.words));
    HIP_TRY(sc->ws.gprtMark.alloc((size_t)P.wsCap));
    rc = gprtBsdfMatrix(sc, P.gprt.lmax, 1024, rd->camera.shutter_open, P.s);
    if (rc) return rc;
  }
  if (P.guides.n) {
    // the side planes, [3 * channels][this plan's batch capacity, which planBatches shrank to fit them, in whole tiles]
    sc->ws.guidesCap = (P.wsCap + 63u) & ~63u;
    HIP_TRY(sc->ws.guides.alloc(3 * (size_t)P.guides.n * (size_t)sc->ws.guidesCap));
  }
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
