// dr_batch.hip -- the batches of dr_render_device (dr_api.hip plans them): BatchRunner (one batch through the stage loop), the loop
// over a plan's batches, and the pilot (the calibration batches of a scene's first big render and the choice they make).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dr_host.h"

using namespace dr_host;

namespace {

// The traversal launches of one calibration batch, per ray kind (the coherent camera launch is every candidate's and is left out).
struct PilotTimes {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];
};

// One batch through the stage loop: gen_samples -> raygen -> trace(camera) -> (guides) -> [shade(b) -> (env) -> trace_closest || trace_any] -> film,
// no host round trips (DirectLighting over mirror / glass: one round of the loop per vertex of a slot's ray tree, one count read back
// per round).  pilot != null: a calibration batch -- a normal batch whose per-lane traversal launches are also collected in pilot->ev.
class BatchRunner {
 public:
  BatchRunner(RenderPlan& plan, Workspace& ws, const int2* pixDev, size_t firstPixel, uint32_t npixels, PilotTimes* pilotTimes)
      : P(plan), sc(plan.sc), rd(plan.rd), rp(plan.rp), L(*plan.L), w(ws), s(plan.s), p0(firstPixel), np(npixels), nslots(npixels * (uint32_t)plan.spp),
        pilot(pilotTimes), C(ws.counters.p) {
    st = makeState(w, P.sf, pixDev, nslots, !P.traits->deviceGenerated && P.needTail > 0, L.stateWords);
    const DrOpt scOpt = dr_opt("DARTRAY_STAGE_COUNTS");
    stageCounts = scOpt.toInt(0) > 0 ? scOpt.toInt(0) : (scOpt.set ? 1 : 0);
    slog.resize(stageCounts ? (size_t)P.nStages + 1 : 0);  // [0] = the camera rays' traversal, [b + 1] = stage b
    // A stage's two traversals are independent (closest hit of the continuation / MIS rays, occlusion of the shadow rays).  Side by
    // side on two streams the any-hit workgroups take the CU slots the closest-hit launch frees as its queue runs dry (a persistent
    // launch ends with its longest rays).  Calibration batches time each launch alone.
    sideBySide = P.overlapAny && !pilot;
  }
  int run();

 private:
  // DARTRAY_STAGE_COUNTS=1 (diagnostics): per stage the list lengths, the kernel times (this batch's own events) and -- with
  // DARTRAY_STAGE_COUNTS=2, which waits for the device after every stage -- the node visits / triangle tests of its traversals
  struct StageLog {
    hipEvent_t s0 = nullptr, sMid = nullptr, s1 = nullptr, c0 = nullptr, c1 = nullptr, a0 = nullptr, a1 = nullptr;
    TraceCounters ctr;
  };
  int loadSamples();
  int loadHostSamples();
  void genBounce(int b);
  hipEvent_t timed(TimedKind kind, hipEvent_t e0);
  hipEvent_t trace(const uint32_t* queue, const uint32_t* nQ, int any, hipStream_t ts, uint32_t* spill, hipEvent_t after = nullptr, bool coherent = false);
  void logTrace(StageLog& g, int any);
  void readCtrNow(TraceCounters* c);
  StageQueues stageQueues(int b, const uint32_t* roundQ, const uint32_t* nRound);
  GprtArgs gprtArgs() const;  // glossy PRT: the side buffers and the scene's tables
  int stage(int b, int round, const uint32_t* roundQ, const uint32_t* nRound);
  int specRound(int round, const uint32_t*& roundQ, const uint32_t*& nRound, bool& done);
  void guides();
  int finish();
  int printStageLog();

  RenderPlan& P;
  DrScene* sc;
  const DrRenderDesc* rd;
  const RenderParams& rp;
  const LayoutOps& L;
  Workspace& w;
  hipStream_t s;
  size_t p0;
  uint32_t np, nslots;
  PilotTimes* pilot;
  uint32_t* C;  // the workspace's counters (CounterLayout)
  BatchState st;
  // The state as the shade stages see it: st itself, but a Halton batch's pixel array is the slots' KEY pixels (k_gen_halton): the streams
  // of the draws inside Li are keyed by the sample's sequence index, not by the pixel it is anchored in
  BatchState shadeState() const {
    BatchState s2 = st;
    if (P.sampler == SamplerKind::Halton) s2.pix = w.halton.keyPix.p;
    return s2;
  }
  uint32_t nGroups = 0;  // lazy generation: 64-pixel groups of this batch
  int wc = 0;            // trace launches of this round so far: each has its own work counters (CounterLayout::workCounters)
  int stageCounts = 0;
  bool sideBySide = false;
  std::vector<StageLog> slog;
  hipEvent_t guides0 = nullptr, guides1 = nullptr;  // k_guides' launch (a guide render's batch), for the stage log
  TraceCounters ctrBase = {};
};

hipEvent_t BatchRunner::timed(TimedKind kind, hipEvent_t e0) {
  hipEvent_t e1 = sc->getEvent();
  (void)hipEventRecord(e1, s);
  sc->traceEvents.push_back({e0, e1, kind});
  return e1;
}

void BatchRunner::readCtrNow(TraceCounters* c) {
  if (stageCounts < 2) return;
  (void)hipStreamSynchronize(s);
  if (sc->s3) (void)hipStreamSynchronize(sc->s3);
  (void)hipMemcpy(c, sc->ctr.p, sizeof(TraceCounters), hipMemcpyDeviceToHost);
}

// lazy sample generation: the LD blocks of bounce b (light number, light component, light position, BSDF direction, path direction:
// the bits genMask gives the level) for the 64-pixel groups marked in alive[b]
void BatchRunner::genBounce(int b) {
  uint64_t m = (15ull << (3 + 4 * b)) | (7ull << (3 + rp.n1D + 3 * b));
  m &= rp.genMask;
  if (!m) return;
  hipEvent_t e0 = sc->getEvent();
  (void)hipEventRecord(e0, s);
  RenderParams rpB = rp;
  rpB.genMask = m;
  BatchState stB = st;
  stB.genAlive = w.alive.p + (size_t)b * nGroups;
  stB.markAlive = nullptr;
  L.gen_samples(rpB, stB, np, s);
  timed(TimedKind::Gen, e0);
}

// Host-buffer sampler: this batch's sample vectors (and the RNG tail) from the caller's memory.
int BatchRunner::loadHostSamples() {
  const int spp = P.spp;
  HIP_TRY(w.aosSamples.alloc((size_t)((P.cap + 63u) & ~63u) * rd->sample_stride));
  HIP_TRY(hipMemcpyAsync(w.aosSamples.p, rd->sample_vec + (size_t)p0 * spp * rd->sample_stride, (size_t)nslots * rd->sample_stride * sizeof(float),
                         hipMemcpyHostToDevice, s));
  L.transpose_samples(w.aosSamples.p, rd->sample_stride, st, rp.nFloats, s);
  if (P.needTail > 0 && P.packedTail) {
    // the batch's runs are one contiguous piece of the packed array: [off[first], off[first + nslots]).  The header promises
    // non-decreasing offsets and runs of at most max_tail values; a host that breaks the promise gets DR_ERR_INVALID here, not a
    // device read outside the piece that is copied (tailOff[slot + 1] - tailOff[slot] as a huge unsigned run).
    const uint64_t* off = rd->tail_offsets + (size_t)p0 * spp;
    for (uint32_t i = 0; i < nslots; ++i)
      if (off[i + 1] < off[i] || off[i + 1] - off[i] > (uint64_t)rd->max_tail)
        return fail(DR_ERR_INVALID, "host-buffer sampler: tail_offsets must be non-decreasing with runs of at most max_tail values");
    const uint64_t o0 = off[0], o1 = off[nslots];
    HIP_TRY(w.tail.alloc((size_t)(o1 - o0) + (size_t)rd->max_tail + 1));
    HIP_TRY(w.tailOff.alloc((size_t)nslots + 1));
    if (o1 > o0) HIP_TRY(hipMemcpyAsync(w.tail.p, rd->tail + o0, (size_t)(o1 - o0) * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.tailOff.p, off, ((size_t)nslots + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    st.tail = w.tail.p;
    st.tailOff = w.tailOff.p;
    st.tailBase = o0;
  } else if (P.needTail > 0) {
    HIP_TRY(hipMemcpyAsync(w.tail.p, rd->tail + (size_t)p0 * spp * rd->max_tail, (size_t)nslots * rd->max_tail * sizeof(double), hipMemcpyHostToDevice, s));
  }
  return DR_OK;
}

// The batch's pixel samples (host buffers, or the device LD sampler: everything now, or lazily) and its camera rays.
int BatchRunner::loadSamples() {
  hipEvent_t evGen = sc->getEvent();
  (void)hipEventRecord(evGen, s);
  if (!P.traits->deviceGenerated) {
    const int rc = loadHostSamples();
    if (rc) return rc;
  } else if (P.lazyGen) {
    // the image (+ lens) blocks for every pixel now; the blocks of bounce b once it is known which 64-pixel groups still have a path there
    RenderParams rpA = rp;
    rpA.genMask = rp.genMask & 3ull;
    L.gen_samples(rpA, st, np, s);
    nGroups = (np + 63u) / 64u;
    HIP_TRY(w.alive.alloc(3 * (size_t)nGroups));
    HIP_TRY(hipMemsetAsync(w.alive.p, 0, 3 * (size_t)nGroups, s));
    sc->genDoneHost += (unsigned long long)np * (unsigned)__builtin_popcountll(rpA.genMask);
    sc->genNamed += (unsigned long long)np * (unsigned)__builtin_popcountll(rp.genMask);
    st.markAlive = w.alive.p;  // k_trace_pk: the groups whose camera rays hit something
    st.markShift = (uint32_t)rp.sppShift + 6u;
  } else {
    P.genSamples(rp, st, np);
    if (P.sf.compact && rp.genMask) {
      sc->genDoneHost += (unsigned long long)np * (unsigned)__builtin_popcountll(rp.genMask);
      sc->genNamed += (unsigned long long)np * (unsigned)__builtin_popcountll(rp.genMask);
    }
  }
  L.raygen(rp, st, s);
  timed(TimedKind::Gen, evGen);
  return DR_OK;
}

// One traversal launch over a queue (null: the batch's slots in order = the camera rays).  Returns its end event.
hipEvent_t BatchRunner::trace(const uint32_t* queue, const uint32_t* nQ, int any, hipStream_t ts, uint32_t* spill, hipEvent_t after, bool coherent) {
  hipEvent_t e0 = sc->getEvent(), e1 = sc->getEvent();
  (void)hipEventRecord(e0, ts);
  bool tookCoherent = false;
  if (!(coherent && L.trace_coherent(sc->d, st, queue, nQ, any, C + CounterLayout::workCounters(wc), sc->ctr.p, P.tgrid, ts))) {
    L.trace(sc->d, st, queue, nQ, any, spill, C + CounterLayout::workCounters(wc++), sc->ctr.p, P.tgrid, ts);
    // (lazy sample generation counts on k_trace_pk's marks: should the coherent kernel ever decline a launch that was to leave
    // them, every group counts as alive -- all blocks are generated, nothing is skipped)
    if (coherent && !any && st.markAlive) (void)hipMemsetAsync(st.markAlive, 1, nGroups, ts);
  } else {
    ++wc;  // (k_trace_pk took this queue: the camera rays)
    tookCoherent = true;
  }
  (void)hipEventRecord(e1, ts);
  // (the pilot compares the per-lane kernels: the coherent camera launch is the same kernel for every candidate and would only
  // compress the ratios its thresholds look at)
  if (pilot && !tookCoherent) pilot->ev[any].push_back({e0, e1});
  sc->traceEvents.push_back({e0, e1, any ? TimedKind::Any : (tookCoherent ? TimedKind::CoherentCamera : TimedKind::Closest), after});
  return e1;
}

void BatchRunner::logTrace(StageLog& g, int any) {
  (any ? g.a0 : g.c0) = sc->traceEvents.back().e0;
  (any ? g.a1 : g.c1) = sc->traceEvents.back().e1;
}

GprtArgs BatchRunner::gprtArgs() const {
  return GprtArgs{P.rounds.nSamples, P.gprt.lmax, P.wsCap, (uint32_t)P.gprt.words, w.gprtBits.p, w.gprtMark.p, sc->prt.K.p, sc->prt.cin.p, sc->gprt.B.p};
}

StageQueues BatchRunner::stageQueues(int b, const uint32_t* roundQ, const uint32_t* nRound) {
  StageQueues q;
  auto cnt = [&](int j, int stg) { return C + CounterLayout::stageCount(j, stg); };
  q.activeIn = b == 0 ? roundQ : ((b - 1) & 1 ? w.activeB.p : w.activeA.p);
  q.nActiveIn = b == 0 ? nRound : cnt(0, b - 1);
  q.activeOut = (b & 1) ? w.activeB.p : w.activeA.p;
  q.nActiveOut = cnt(0, b);
  q.closestQ = w.closestQ.p;
  q.nClosest = cnt(1, b);
  q.anyQ = w.anyQ.p;
  q.nAny = cnt(2, b);
  q.work = cnt(3, b);
  q.ctr = sc->ctr.p;
  q.envQ = P.envStage ? w.envQ.p : nullptr;
  q.nEnv = C + CounterLayout::envCount(b);
  return q;
}

// Stage b: shade the active list (+ the environment-map kernel), generate the next bounce's sample blocks where paths are alive,
// trace the continuation / MIS rays and the shadow rays the stage queued.
int BatchRunner::stage(int b, int round, const uint32_t* roundQ, const uint32_t* nRound) {
  StageQueues q = stageQueues(b, roundQ, nRound);
  const bool log = stageCounts && round == 0;
  // ambient occlusion, the last stage of a round that another one follows: its output list -- the slots that hit, every one with rays still
  // to send -- is the next round's input and must outlive the reset of the stage counters: it goes to a round list and a round word
  if (b + 1 == P.nStages && round + 1 < P.shadowRounds()) {
    q.activeOut = (round & 1) ? w.roundB.p : w.roundA.p;
    q.nActiveOut = C + CounterLayout::roundNext(round);
    HIP_TRY(hipMemsetAsync(q.nActiveOut, 0, sizeof(uint32_t), s));
  }
  hipEvent_t evS = sc->getEvent();
  (void)hipEventRecord(evS, s);
  const BatchState stS = shadeState();
  // the integrator's shading launcher, and the rays it queues: closest-hit (continuation / MIS) and any-hit (shadow) rays, or -- a Whitted stage --
  // one shadow ray per slot and nothing else (no MIS ray, no continuation: the child rays are the rounds')
  bool shadowRaysOnly = false;
  // the integrators whose rays go in rounds (Rounds; zeros under every other), stage b of round `round`: ray b - 1 of the round folded in, ray b
  // queued (the last stage only folds)
  const Rounds& R = P.rounds;
  const int folded = b > 0 ? round * R.perRound + b - 1 : -1, queued = b < R.perRound ? round * R.perRound + b : -1;
  switch (P.integrator) {  // (no default: -Wall names a kind this forgets)
    case IntegratorKind::Path: L.shade_path(sc->d, rp, stS, q, b, P.sgrid, s); break;
    case IntegratorKind::DirectAll: case IntegratorKind::DirectOne: L.shade_direct(sc->d, rp, stS, q, b, P.sgrid, s); break;
    case IntegratorKind::Whitted: L.shade_whitted(sc->d, rp, stS, q, b, P.sgrid, s); shadowRaysOnly = true; break;
    case IntegratorKind::AmbientOcclusion:
      L.shade_ao(sc->d, rp, stS, q, R.nSamples, folded, queued, P.ao.minDist, P.ao.maxDist, P.sgrid, s);
      shadowRaysOnly = true;
      break;
    case IntegratorKind::Feature: L.shade_feature(sc->d, stS, q, P.feature.channel, P.sgrid, s); break;  // (the only stage: nothing is traced behind it)
    case IntegratorKind::DiffusePRT: {  // the stages and rounds of ambient occlusion; the fold adds to the slot's transfer coefficients (Workspace::prt)
      const PrtArgs a = {R.nSamples, P.prt.lmax, P.wsCap, 0u, w.prt.p, sc->prt.K.p, sc->prt.cin.p};
      L.shade_prt(sc->d, rp, stS, q, a, folded, queued, P.sgrid, s);
      shadowRaysOnly = true;
      break;
    }
    case IntegratorKind::GlossyPRT:  // the same stages and rounds; the fold records one visibility bit (Workspace::gprtBits)
      L.shade_gprt(sc->d, rp, stS, q, gprtArgs(), folded, queued, P.sgrid, s);
      if (b + 1 == P.nStages && round + 1 == R.rounds) L.gprt_finish(stS, gprtArgs(), s);  // behind the last fold: the rest of Li, one wave per slot
      shadowRaysOnly = true;
      break;
    case IntegratorKind::UseProbes: {  // (the only stage: nothing is traced behind it)
      const auto& g = sc->probes;
      const ProbeArgs a = {g.lmax, {g.n[0], g.n[1], g.n[2]}, {g.b[0], g.b[1], g.b[2]}, {g.b[3], g.b[4], g.b[5]}, g.cin.p, g.K.p};
      L.shade_probes(sc->d, stS, q, a, P.sgrid, s);
      break;
    }
    case IntegratorKind::Material: L.shade_material(sc->d, stS, q, P.material.channel, P.sgrid, s); break;  // (the only stage: nothing is traced behind it)
  }
  hipEvent_t evMid = nullptr;
  if (stageCounts && P.envStage) {
    evMid = sc->getEvent();
    (void)hipEventRecord(evMid, s);
  }
  if (P.envStage) L.env(sc->d, rp, stS, q, b, P.sgrid, s);
  hipEvent_t evS1 = timed(TimedKind::Shade, evS);
  if (P.lazyGen && round == 0 && b < 2 && b + 1 <= rd->max_depth) {  // bounce b + 1's blocks for the groups in this stage's output list
    L.mark_alive(q.activeOut, q.nActiveOut, (uint32_t)rp.sppShift + 6u, w.alive.p + (size_t)(b + 1) * nGroups, s);
    genBounce(b + 1);
  }
  if (log) {
    slog[b + 1].s0 = evS;
    slog[b + 1].sMid = evMid;
    slog[b + 1].s1 = evS1;
  }
  if (b + 1 >= P.nStages) return DR_OK;
  if (shadowRaysOnly) {
    trace(q.anyQ, q.nAny, 1, s, w.spill.p);
    if (log) logTrace(slog[b + 1], 1);
  } else if (sideBySide) {
    hipEvent_t eS = sc->getEvent(), eA = sc->getEvent();
    (void)hipEventRecord(eS, s);
    (void)hipStreamWaitEvent(sc->s3, eS, 0);
    hipEvent_t closestEnd = trace(q.closestQ, q.nClosest, 0, s, w.spill.p);
    if (log) logTrace(slog[b + 1], 0);
    trace(q.anyQ, q.nAny, 1, sc->s3, w.spill.p + w.spillHalf, closestEnd);
    if (log) logTrace(slog[b + 1], 1);
    (void)hipEventRecord(eA, sc->s3);
    (void)hipStreamWaitEvent(s, eA, 0);
  } else {
    trace(q.closestQ, q.nClosest, 0, s, w.spill.p);
    if (log) logTrace(slog[b + 1], 0);
    trace(q.anyQ, q.nAny, 1, s, w.spill.p);
    if (log) logTrace(slog[b + 1], 1);
  }
  if (log) readCtrNow(&slog[b + 1].ctr);
  return DR_OK;
}

// A guide render, behind the camera rays' traversal and in front of the first shading launch, on the closest-hit stream: the
// slots still hold the hit record and the camera ray -- what the per-lane kernels and k_trace_pk both leave: F_HPRIM and F_HT written, F_RO and F_RD
// as k_raygen stored them -- and k_guides writes every requested channel's value to its side plane.  One launch however many channels.
void BatchRunner::guides() {
  guides0 = sc->getEvent();
  (void)hipEventRecord(guides0, s);
  L.guides(sc->d, st, w.guides.p, w.guidesCap, P.guides.mask, sc->ctr.p, P.sgrid, s);
  guides1 = timed(TimedKind::Guides, guides0);
}

// DirectLighting over mirror / glass, the end of a round: k_shade_spec pops / pushes every slot's frame stack and lists the slots
// whose child ray the next round traces.  done: no slot launched a child.
int BatchRunner::specRound(int round, const uint32_t*& roundQ, const uint32_t*& nRound, bool& done) {
  StageQueues q;
  memset(&q, 0, sizeof(q));
  q.activeIn = roundQ;
  q.nActiveIn = nRound;
  uint32_t* nextQ = (round & 1) ? w.roundB.p : w.roundA.p;
  uint32_t* nNext = C + CounterLayout::roundNext(round);
  HIP_TRY(hipMemsetAsync(nNext, 0, sizeof(uint32_t), s));
  q.activeOut = nextQ;
  q.nActiveOut = nNext;
  q.closestQ = w.closestQ.p;  // unused: the child rays are the next round's list
  q.nClosest = C + CounterLayout::roundClosest;
  q.anyQ = w.anyQ.p;
  q.nAny = C + CounterLayout::roundAny;
  q.ctr = sc->ctr.p;
  hipEvent_t evS = sc->getEvent();
  (void)hipEventRecord(evS, s);
  L.shade_spec(sc->d, rp, shadeState(), q, P.sgrid, s);
  timed(TimedKind::Shade, evS);
  uint32_t live = 0;  // (a synchronous read-back per round: this is not the throughput path)
  HIP_TRY(hipMemcpyAsync(&live, nNext, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  done = live == 0;
  roundQ = nextQ;
  nRound = nNext;
  return DR_OK;
}

int BatchRunner::printStageLog() {
  std::vector<uint32_t> hc(CounterLayout::total);
  HIP_TRY(hipStreamSynchronize(s));
  if (sc->s3) HIP_TRY(hipStreamSynchronize(sc->s3));
  HIP_TRY(hipMemcpy(hc.data(), C, CounterLayout::total * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const size_t batch = (size_t)sc->stats.batches;
  for (int b = 0; b < P.nStages; ++b)
    fprintf(stderr, "stage_counts batch %zu stage %d: in %u active_out %u closest %u any %u env %u\n", batch, b, b == 0 ? nslots : hc[CounterLayout::stageCount(0, b - 1)],
            hc[CounterLayout::stageCount(0, b)], hc[CounterLayout::stageCount(1, b)], hc[CounterLayout::stageCount(2, b)], hc[CounterLayout::envCount(b)]);
  // the kernel times of the same stages (side-by-side any-hit launches overlap the closest-hit ones: DARTRAY_OVERLAP_ANY=0 gives each its
  // own time) and, with DARTRAY_STAGE_COUNTS=2, the traversal work of each stage
  auto ms = [](hipEvent_t a, hipEvent_t b) {
    float t = 0.f;
    return a && b && hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0;
  };
  for (int i = 0; i <= P.nStages; ++i) {
    const StageLog& g = slog[i];
    const double shade = g.sMid ? ms(g.s0, g.sMid) : ms(g.s0, g.s1), env = g.sMid ? ms(g.sMid, g.s1) : 0.0;
    fprintf(stderr, "stage_times batch %zu stage %d: shade %.4f env %.4f closest %.4f any %.4f ms", batch, i - 1, shade, env, ms(g.c0, g.c1), ms(g.a0, g.a1));
    if (stageCounts >= 2 && (i == 0 || g.c0 || g.a0)) {
      const TraceCounters& p = i ? slog[i - 1].ctr : ctrBase;
      fprintf(stderr, "; closest rays %llu nodes %llu tris %llu any rays %llu nodes %llu tris %llu", g.ctr.closest_rays - p.closest_rays,
              g.ctr.closest_nodes - p.closest_nodes, g.ctr.closest_tris - p.closest_tris, g.ctr.any_rays - p.any_rays, g.ctr.any_nodes - p.any_nodes,
              g.ctr.any_tris - p.any_tris);
    }
    fprintf(stderr, "\n");
  }
  if (P.guides.n) {
    float t = 0.f;
    (void)hipEventElapsedTime(&t, guides0, guides1);
    fprintf(stderr, "stage_times batch %zu guides: %d channels (mask 0x%x) %.4f ms\n", batch, P.guides.n, P.guides.mask, (double)t);
  }
  return DR_OK;
}

// After the last stage: the sampler statistics, the film, the diagnostics.
int BatchRunner::finish() {
  if (P.lazyGen) {  // statistics: the (pixel, block) pairs the three genBounce calls came to
    uint32_t nb[3];
    for (int b = 0; b < 3; ++b) nb[b] = (uint32_t)__builtin_popcountll(((15ull << (3 + 4 * b)) | (7ull << (3 + rp.n1D + 3 * b))) & rp.genMask);
    L.sum_alive(w.alive.p, nGroups, np, nb, sc->ctr.p, s);
  }
  hipEvent_t evF = sc->getEvent();
  (void)hipEventRecord(evF, s);
  // adaptive, first pass: the pixels that need maxSamples go to the list and leave this batch's film step (their entries of the
  // render's pixel array, which no later batch reads, move outside every film window)
  if (P.adaptive.pass == 1) L.adaptive_decide(rp, st, np, w.pix.p + p0, w.adaptList.p, w.adaptCount.p, (uint32_t)P.npixTotal, s);
  L.film(rp, st, sc->ws.filterTable.p, np, P.film, s);
  if (P.guides.n) {
    // every channel's side plane through the same film kernel -- the same samples, filter table and window -- into the channel's own film.
    // k_film reads its radiance and its image samples off ONE base pointer (BatchState::tiles), so a plane cannot be handed to it beside the
    // state's sample region: the plane is moved into the state's radiance plane instead, which the beauty film above was the last to read
    // (same stream: behind it).  No deferred light term: the state's flags are the beauty render's
    RenderParams rpG = rp;
    rpG.deferredNee = 0;
    for (int i = 0; i < P.guides.n; ++i) {
      L.guide_plane(st, w.guides.p, w.guidesCap, P.guides.plane[i], P.sgrid, s);
      L.film(rpG, st, sc->ws.filterTable.p, np, P.guides.film[i], s);
    }
  }
  timed(TimedKind::Film, evF);
  sc->stats.batches++;
  if (stageCounts) {
    const int rc = printStageLog();
    if (rc) return rc;
  }
  HIP_TRY(hipGetLastError());
  if (!P.traits->deviceGenerated) HIP_TRY(hipStreamSynchronize(s));  // host buffers of the next batch reuse the staging area
  return DR_OK;
}

int BatchRunner::run() {
  // a guide render: the one contract of k_guides and of the film step's k_guide_plane launches, which check nothing themselves -- the side
  // planes exist, hold this batch's slots, and every channel's plane is one of them
  if (P.guides.n) {
    if (!w.guides.p || nslots > w.guidesCap || (size_t)3 * P.guides.n * w.guidesCap > w.guides.n)
      return fail(DR_ERR_HIP, "render guides: a batch larger than the side planes were sized for");
    for (int i = 0; i < P.guides.n; ++i)
      if (P.guides.plane[i] < 0 || P.guides.plane[i] >= P.guides.n || !P.guides.film[i]) return fail(DR_ERR_INVALID, "render guides: a channel without a plane or a film");
  }
  HIP_TRY(hipMemsetAsync(C, 0, CounterLayout::total * sizeof(uint32_t), s));
  int rc = loadSamples();
  if (rc) return rc;
  // DirectLighting over mirror / glass: one round of the stage loop per vertex of a slot's ray tree (at most 2^maxDepth rounds, like the
  // recursion itself); `roundQ` lists the slots whose (camera or child) ray this round traces.  Everything else: one round.
  const uint32_t* roundQ = nullptr;
  const uint32_t* nRound = nullptr;
  if (P.dlSpec) HIP_TRY(hipMemsetAsync(w.specSp.p, 0, (size_t)w.cap * sizeof(int32_t), s));
  for (int round = 0;; ++round) {
    if (round > 0) {  // the stage counters are reused every round; the round lists' counts live behind them
      for (const CounterLayout::Range& r : CounterLayout::roundReset) HIP_TRY(hipMemsetAsync(C + r.offset, 0, r.length * sizeof(uint32_t), s));
      wc = 0;
    }
    if (stageCounts && round == 0) readCtrNow(&ctrBase);
    // camera rays (or this round's child rays; a later round of ambient occlusion has none: its slots go on with their occlusion rays)
    if (round == 0 || P.dlSpec) trace(roundQ, nRound, 0, s, w.spill.p, nullptr, P.coherentCamera && roundQ == nullptr);
    if (stageCounts && round == 0) {  // (before genBounce pushes its own event)
      logTrace(slog[0], 0);
      readCtrNow(&slog[0].ctr);
    }
    if (P.guides.n && round == 0) guides();  // (before anything shades: the first shading launch overwrites the camera ray)
    if (P.lazyGen && round == 0) {
      st.markAlive = nullptr;
      genBounce(0);
    }
    for (int b = 0; b < P.nStages; ++b) {
      rc = stage(b, round, roundQ, nRound);
      if (rc) return rc;
    }
    if (round + 1 < P.shadowRounds()) {  // ambient occlusion, diffuse PRT: the next 128 rays of every slot that hit (no count read back: the rounds are known)
      roundQ = (round & 1) ? w.roundB.p : w.roundA.p;
      nRound = C + CounterLayout::roundNext(round);
      continue;
    }
    if (!P.dlSpec) break;
    bool done = false;
    rc = specRound(round, roundQ, nRound, done);
    if (rc) return rc;
    if (done) break;
  }
  return finish();
}

// The choice, from the calibration batches' times per algorithmic byte.
void pickTraceKernels(DrScene* sc, const PilotResult& R) {
  const double(&perByte)[2][3] = R.perByte;
  for (int kind = 0; kind < 2; ++kind)
    for (int c = 0; c < 3; ++c) {
      sc->calibMs[kind][c] = R.ms[kind][c];
      sc->calibPerGB[kind][c] = (float)perByte[kind][c];
    }
  // closest-hit rays: a pair kernel needs 5 % on k_trace<0>
  sc->d.traceKernel[0] = perByte[0][1] < 0.95 * perByte[0][0] ? 3u : 2u;
  // ... and has a second form (round 4): the cold ray state in LDS, six workgroups per CU -- at full size 2.5 - 3 % ahead of k_trace3<0>
  // on C5 (728 against 762 - 786 ms) and level on C4 (123.2 / 123.5), while the calibration batches put it anywhere from 2 % behind to
  // 1 % ahead: it keeps the pair family's place unless k_trace3<0> beats it by 5 % there
  if (perByte[0][2] > 0.0) {
    const double best3 = std::min(perByte[0][1], perByte[0][2]);
    if (best3 < 0.95 * perByte[0][0]) sc->d.traceKernel[0] = perByte[0][2] < 1.05 * perByte[0][1] ? 5u : 3u;
  }
  // The any-hit rays.  Their calibration launches are the least reliable of the pilot -- shadow rays are short, a small launch is
  // mostly ramp-up and tail, and the two families come out within a few per cent of each other on the cache-resident scenes (C2:
  // k_trace3a 6 - 12 % ahead in the calibration batches of five boxes, level at full size) while small launches understate the pair
  // kernel on the big incoherent tree (C4: -2 ... +6 % in a calibration batch, +25 % at full size).  So they stay in the FAMILY the
  // closest-hit rays chose -- k_trace<1> beside k_trace<0>, k_trace3a beside k_trace3<0> / k_trace3c -- and cross over only when
  // their own calibration batch says so by more than 15 %.
  const bool pairFamily = sc->d.traceKernel[0] != 2u;
  const double own = pairFamily ? perByte[1][1] : perByte[1][0], other = pairFamily ? perByte[1][0] : perByte[1][1];
  const bool cross = other > 0.0 && own > 0.0 && other < 0.85 * own;
  sc->d.traceKernel[1] = (pairFamily != cross) ? 3u : 2u;
  // ... and their visit ORDER (round 6): intersectP's boolean does not depend on it (bvh_accel.dart:167-226 never touches the ray), the work
  // of a ray that finds an occluder does.  The pilot's first batch -- the cache warm-up -- ran its any-hit rays far child first, the second
  // in the reference order, both through k_trace<1>: where the far child first is cheaper per ray even in the cold batch (ratio below
  // 0.97), the scene's any-hit rays take it -- in whichever kernel family they run (the order is a property of the rays and the tree).
  // Measured at full size, kernels forced (profiles/r06_far_first_ab.txt): C5 (the courtyard under the sky: 42 % of the shadow rays are
  // occluded and visit 35 % fewer nodes) any-hit 505.8 -> 398.9 ms, 1180 -> 1254 Msamples/s; C2 96.8 -> 93.1 ms and C4 101.0 -> 98.2 ms
  // although their occluded rays visit 11 - 13 % MORE nodes that way -- they test 3 - 4 % fewer triangles, and an f64 triangle test costs
  // several node visits.  Pilot ratios of the same boxes: C5 0.62, C2 0.90, C4 0.94.
  sc->calibFarFirst = R.anyMsPerRayRef > 0.0 ? (float)(R.anyMsPerRayFar / R.anyMsPerRayRef) : 0.f;
  if (R.anyMsPerRayRef > 0.0 && R.anyMsPerRayFar > 0.0 && R.anyMsPerRayFar < 0.97 * R.anyMsPerRayRef) sc->d.traceKernel[1] = sc->d.traceKernel[1] == 3u ? 7u : 6u;
  sc->traceCalibrated = true;
}

}  // namespace

namespace dr_host {

// The ordinary batches of a plan: its pixels from firstPixel on (pixDev: the plan's pixel array on the device).
int runBatches(RenderPlan& plan, const int2* pixDev, size_t firstPixel) {
  for (size_t p0 = firstPixel; p0 < plan.npixTotal; p0 += plan.pixPerBatch) {
    const uint32_t np = (uint32_t)std::min<size_t>(plan.pixPerBatch, plan.npixTotal - p0);
    const int rc = BatchRunner(plan, plan.sc->ws, pixDev + p0, p0, np, nullptr).run();
    if (rc) return rc;
  }
  return DR_OK;
}

int haltonSelect(RenderPlan& P, uint64_t k0, uint32_t n, uint32_t* accepted) {
  Workspace& w = P.sc->ws;
  P.L->halton_select(P.halton.win, k0, n, w.halton.blk.p, w.halton.idx.p, P.s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(accepted, w.halton.blk.p + (n + 255u) / 256u, sizeof(uint32_t), hipMemcpyDeviceToHost, P.s));
  HIP_TRY(hipStreamSynchronize(P.s));
  return DR_OK;
}

// The batches of a Halton render: equal ranges of the sequence's indices.  Per batch: the selection, its count read back, then an
// ordinary batch of that many slots whose sample generation (RenderPlan::genSamples) also writes the slots' anchor pixels.
int runHaltonBatches(RenderPlan& P, uint64_t* acceptedTotal) {
  DrScene* sc = P.sc;
  *acceptedTotal = 0;
  for (uint64_t k0 = 0; k0 < P.npixTotal; k0 += P.pixPerBatch) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(P.pixPerBatch, P.npixTotal - k0);
    hipEvent_t e0 = sc->getEvent(), e1 = sc->getEvent();
    (void)hipEventRecord(e0, P.s);
    uint32_t accepted = 0;
    int rc = haltonSelect(P, k0, n, &accepted);
    if (rc) return rc;
    (void)hipEventRecord(e1, P.s);
    sc->traceEvents.push_back({e0, e1, TimedKind::Gen});
    if (accepted > n) return fail(DR_ERR_HIP, "halton sampler: the selection accepted more indices than its range holds");
    *acceptedTotal += accepted;
    if (accepted == 0) continue;
    rc = BatchRunner(P, sc->ws, sc->ws.pix.p, 0, accepted, nullptr).run();
    if (rc) return rc;
  }
  return DR_OK;
}

int runPilot(RenderPlan& P, PilotResult& R) {
  DrScene* sc = P.sc;
  hipStream_t s = P.s;
  hipEvent_t evP0 = sc->getEvent(), evP1 = sc->getEvent();
  HIP_TRY(hipEventRecord(evP0, s));
  auto readCtr = [&](TraceCounters* c) -> int {
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(c, sc->ctr.p, sizeof(TraceCounters), hipMemcpyDeviceToHost));
    return DR_OK;
  };
  const uint32_t keepKernel[2] = {sc->d.traceKernel[0], sc->d.traceKernel[1]};
  auto abandon = [&](int code) {  // an error in the middle: the scene keeps the choice it had, not a forced one
    sc->d.traceKernel[0] = keepKernel[0];
    sc->d.traceKernel[1] = keepKernel[1];
    return code;
  };
  for (int set = 0; set < P.pilotSets; ++set) {  // warm-up (k_trace), k_trace timed, k_trace3 timed, k_trace3c timed (its any-hit rays: k_trace3a again)
    // where the pair kernel has just lost clearly to k_trace<0> (C2: 8 - 10 % behind) its cold-state sibling is not timed: k_trace3c is
    // never more than a few per cent from k_trace3<0>, and the batch is a quarter of the pilot's cost.  Its pixels stay in the ordinary batches.
    if (set == 3 && P.calibrateTrace && R.perByte[0][1] > 1.05 * R.perByte[0][0]) break;
    ++R.setsRun;
    const int impl = set == 2 ? 3 : (set == 3 ? 5 : 2);
    const int col = set == 2 ? 1 : (set == 3 ? 2 : 0);
    if (P.calibrateTrace) {
      sc->d.traceKernel[0] = (uint32_t)impl;
      sc->d.traceKernel[1] = impl == 5 ? 3u : (set == 0 ? 6u : (uint32_t)impl);  // (the warm-up batch: k_trace<1> far child first, see pickTraceKernels)
    }
    TraceCounters c0, c1;
    int prc = readCtr(&c0);
    if (prc) return abandon(prc);
    PilotTimes pt;
    prc = BatchRunner(P, sc->ws, sc->ws.pix.p + set * P.calibPix, set * P.calibPix, (uint32_t)P.calibPix, &pt).run();
    if (prc) return abandon(prc);
    prc = readCtr(&c1);
    if (prc) return abandon(prc);
    if (set == 0 && P.measureLayout) {
      // the batch's stage lists (still in the counters): how many of its slots are alive at the second bounce?
      uint32_t alive2 = 0;
      if (hipMemcpy(&alive2, sc->ws.counters.p + CounterLayout::stageCount(0, 1), sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)  // entries of stage 1's output list
        return abandon(fail(DR_ERR_HIP, "layout pilot: counter read-back failed"));
      sc->layoutDensity = (float)((double)alive2 / ((double)P.calibPix * P.spp));
      sc->stateLayout = sc->layoutDensity < 0.5f ? 4 : 64;
      P.L = sc->stateLayout == 4 ? &kLayoutSp4 : &kLayout64;
      if (dr_opt("DARTRAY_VERBOSE"))
        fprintf(stderr, "dartray_hip: state-layout pilot: %.3f of a batch's slots alive at the second bounce -> %s\n", sc->layoutDensity,
                sc->stateLayout == 4 ? "four-slot line-grouped sub-tiles (sp4)" : "64-slot runs");
    }
    if (P.calibrateTrace && set <= 1) {  // any-hit time per ray, far child first (batch 0) against the reference order (batch 1)
      float sum = 0.f;
      for (auto& e : pt.ev[1]) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e.first, e.second);
        sum += t;
      }
      const double rays = (double)(c1.any_rays - c0.any_rays);
      (set == 0 ? R.anyMsPerRayFar : R.anyMsPerRayRef) = rays > 0.0 ? (double)sum / rays : 0.0;
    }
    if (set == 0 || !P.calibrateTrace) continue;
    // the per-lane kernels' own work: the batch's totals without what k_trace_pk traced of them (the camera rays)
    const double bytes[2] = {32.0 * (double)((c1.closest_nodes - c0.closest_nodes) - (c1.pk_nodes[0] - c0.pk_nodes[0])) +
                                 48.0 * (double)((c1.closest_tris - c0.closest_tris) - (c1.pk_tris[0] - c0.pk_tris[0])),
                             32.0 * (double)(c1.any_nodes - c0.any_nodes) + 48.0 * (double)(c1.any_tris - c0.any_tris)};
    for (int kind = 0; kind < 2; ++kind) {
      float sum = 0.f;
      for (auto& e : pt.ev[kind]) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e.first, e.second);
        sum += t;
      }
      R.ms[kind][col] = sum;
      R.perByte[kind][col] = bytes[kind] > 0.0 ? (double)sum / (bytes[kind] * 1.0e-9) : 0.0;
    }
  }
  if (P.calibrateTrace) pickTraceKernels(sc, R);
  HIP_TRY(hipEventRecord(evP1, s));
  sc->traceEvents.push_back({evP0, evP1, TimedKind::Pilot});  // DrRenderStats.pilot_ms: the time of the calibration batches
  if (P.calibrateTrace && dr_opt("DARTRAY_VERBOSE"))
    fprintf(stderr, "dartray_hip: traversal pilot (%d x %zu samples, rendered into the film), ms per algorithmic GB of the per-lane kernels: closest v2 %.4f / v3 %.4f / v3c %.4f -> v%u; "
            "any hit v2 %.4f / v3 %.4f, far child first / reference order per ray %.3f -> v%u\n", R.setsRun, P.calibPix * (size_t)P.spp, R.perByte[0][0], R.perByte[0][1], R.perByte[0][2], sc->d.traceKernel[0],
            R.perByte[1][0], R.perByte[1][1], sc->calibFarFirst, sc->d.traceKernel[1]);
  return DR_OK;
}

}  // namespace dr_host
