// dr_shade_loop.h -- the two loop shapes of the shading units outside dr_kernels.hip, written once: the queue-fed stage
// loop (StageLoop, stage_loop_begin / _slot / _push / _end) and the one-lane-per-slot kernels' epilogue and launcher (per_slot_begin / _end,
// launch_per_slot).
// Included INSIDE the unit's layout namespace (DR_NS), behind dr_kernels.h, dr_wave.h and dr_shade_common.h (shade_count): includes nothing itself.
#ifndef DR_SHADE_LOOP_H
#define DR_SHADE_LOOP_H

// ---- the queue-fed stage loop: a kernel that takes its slots from the stage's input list and queues rays and survivors ----
//   StageLoop loop = stage_loop_begin(s_push, st, q);
//   for (uint32_t it = 0; it < loop.nIter; ++it) {
//     uint32_t slot = 0; ...
//     if (stage_loop_slot(loop, q, it, &slot)) { ...the slot's work... }
//     stage_loop_push(s_push, loop, q, it, ...what to queue...);     // every lane, valid or not: the push is wave-wide
//   }
//   stage_loop_end(s_push, loop, q);
struct StageLoop {
  PushCtx pctx;
  uint32_t nIn, stride, nIter;
};
DR_DEV StageLoop stage_loop_begin(PushStage& sm, const BatchState& st, const StageQueues& q) {
  StageLoop l;
  l.pctx = PushCtx{{0, 0, 0, 0}, 0, 0};
  l.nIn = q.nActiveIn ? *q.nActiveIn : st.nslots;
  l.stride = gridDim.x * blockDim.x;
  l.nIter = (l.nIn + l.stride - 1) / l.stride;
  stage_init(sm);
  return l;
}
DR_DEV bool stage_loop_slot(const StageLoop& l, const StageQueues& q, uint32_t it, uint32_t* slot) {
  const uint32_t idx = it * l.stride + blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= l.nIn) return false;
  *slot = q.activeIn ? q.activeIn[idx] : idx;
  return true;
}
DR_DEV void stage_loop_push(PushStage& sm, StageLoop& l, const StageQueues& q, uint32_t it, bool pCont, bool pMis, bool pAny, bool pAct,
                            uint32_t slot, uint32_t misBit, bool pVert) {
  stage_push(sm, l.pctx, pCont, pMis, pAny, pAct, slot, misBit, pVert);
  if (l.pctx.iters == DR_PUSH_ITERS || it + 1 == l.nIter)
    stage_flush(sm, l.pctx, q.closestQ, q.nClosest, q.anyQ, q.nAny, q.activeOut, q.nActiveOut, &q.ctr->shade_cont);
}
DR_DEV void stage_loop_end(PushStage& sm, StageLoop& l, const StageQueues& q) {
  stage_finish(sm, l.pctx, q.closestQ, q.anyQ, q.activeOut, &q.ctr->shade_cont);
  shade_count(sm, q.ctr, l.nIn);
}

// ---- the one-lane-per-slot kernels: slots in order, nothing queued ----
// DrRenderStats.shade_items / shade_vertices, as shade_count keeps them: one atomic per workgroup.  The kernel owns the LDS word
// (`__shared__ uint32_t s_hits;`), zeroes it with per_slot_begin before its slot loop -- where the barrier's wait hides behind the
// first loads; zeroing it behind the loop cost k_shade_probes 3 % (MEASUREMENTS.md) -- and hands each lane's count of camera hits to
// per_slot_end behind the loop.  Both are called once, by every thread.
DR_DEV void per_slot_begin(uint32_t& s_hits) {
  if (threadIdx.x == 0) s_hits = 0u;
  __syncthreads();
}
DR_DEV void per_slot_end(uint32_t& s_hits, uint32_t hits, TraceCounters* ctr, uint32_t nslots) {
  if (hits) atomicAdd(&s_hits, hits);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_hits) atomicAdd(&ctr->shade_vertices, (unsigned long long)s_hits);
    if (blockIdx.x == 0) atomicAdd(&ctr->shade_items, (unsigned long long)nslots);
  }
}
// grid: the CUs; at most 8 workgroups of BLOCK threads each, fewer when the slots need fewer
template <auto kernel, int BLOCK, class... A>
static void launch_per_slot(int grid, uint32_t nslots, hipStream_t s, A... args) {
  if (nslots == 0) return;
  const unsigned need = (nslots + BLOCK - 1) / BLOCK, most = (unsigned)grid * 8u;
  hipLaunchKernelGGL(kernel, dim3(need < most ? need : most), dim3(BLOCK), 0, s, args...);
}

#endif
