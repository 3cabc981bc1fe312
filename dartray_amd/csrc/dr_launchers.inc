// Launchers of the kernels in dr_kernels.hip / dr_trace.hip.  Included by dr_kernels.h twice: at global scope (the default state
// layout, DR_SUB = 64) and inside namespace sp4 (the same sources compiled with -DDR_SUB=4 -DDR_NS=sp4: sub-tiles of four slots,
// for renders whose stage lists thin out -- see dr_kernels.h and MEASUREMENTS.md, round 3).
void launch_gather_tris(const float* verts, const uint32_t* idx, const uint32_t* mat, const int32_t* light,
                        const uint8_t* rev, float4* out, uint64_t ntris, hipStream_t s);
void launch_make_shtris(const DScene& sc, float4* out, uint64_t ntris, hipStream_t s);
void launch_intersect(const DScene& sc, const DrRay* rays, int64_t n, DrHit* out, int anyHit, uint32_t* spill,
                      uint32_t* workCounter, TraceCounters* ctr, int grid, hipStream_t s, int forceImpl = 0);
void launch_trace(const DScene& sc, const BatchState& st, const uint32_t* queue, const uint32_t* nQueue, int anyHit,
                  uint32_t* spill, uint32_t* workCounter, TraceCounters* ctr, int grid, hipStream_t s);
bool launch_trace_coherent(const DScene& sc, const BatchState& st, const uint32_t* queue, const uint32_t* nQueue, int anyHit, uint32_t* workCounter,
                           TraceCounters* ctr, int grid, hipStream_t s);
// the kernel launch_trace would pick right now for this scene and ray kind, as a kernel id (1 / 2 / 3 / 5; switches included)
int trace_kernel_id(const DScene& sc, int anyHit);
void launch_gen_samples(const RenderParams& rp, const BatchState& st, uint32_t npix, hipStream_t s);
// dr_sampler_strat.hip: the stratified device sampler (xsamples x spp / xsamples strata; jitter: rp.samplerMode) and dr_generate_samples' dump
void launch_gen_strat(const RenderParams& rp, const BatchState& st, uint32_t npix, int xsamples, hipStream_t s);
void launch_export_samples(const RenderParams& rp, const BatchState& st, float* out, int stride, hipStream_t s);
// dr_sampler_adaptive.hip: AdaptiveSampler.needsSupersampling for the npix pixels of a first-pass batch, in front of its film step --
// flagged pixels are appended to list (counts[0]: its length, counts[1]: those inside the film window) and retired from pix
void launch_adaptive_decide(const RenderParams& rp, const BatchState& st, uint32_t npix, int2* pix, int2* list, uint32_t* counts,
                            uint32_t listCap, hipStream_t s);
// dr_sampler_halton.hip (DR_SAMPLER_HALTON).  win[5] = the task's window as HaltonSampler holds it: left, top, right, bottom (inclusive,
// sampler.dart:52-54), delta = max(width, height).  launch_halton_select: the indices of [k0, k0 + n) of the task's sequence that fall inside the
// window, in increasing order, to seqIdx (room for n); blk: (n + 255) / 256 + 1 words, the last receives their number.  launch_gen_halton: the
// st.nslots accepted samples' float-form vectors, their anchor pixels (pix[slot]: k_raygen, k_film) and their KEY pixels (keyPix[slot]: the pixel
// whose index in the sampler extent is the sample's sequence index -- what the in-Li streams of the shade kernels are keyed by)
void launch_halton_select(const int32_t win[5], uint64_t k0, uint32_t n, uint32_t* blk, unsigned long long* seqIdx, hipStream_t s);
void launch_gen_halton(const RenderParams& rp, const BatchState& st, const int32_t win[5], const unsigned long long* seqIdx, int2* pix, int2* keyPix,
                       hipStream_t s);
// dr_sampler_random.hip (DR_SAMPLER_RANDOM): the st.nslots float-form vectors of the batch, every value one randomFloat() of the slot's own stream
void launch_gen_random(const RenderParams& rp, const BatchState& st, hipStream_t s);
void launch_mark_alive(const uint32_t* list, const uint32_t* nList, uint32_t shift, uint8_t* alive, hipStream_t s);
void launch_sum_alive(const uint8_t* alive, uint32_t nGroups, uint32_t npix, const uint32_t nb[3], TraceCounters* ctr, hipStream_t s);
void launch_transpose_samples(const float* aos, int stride, const BatchState& st, int nFloats, hipStream_t s);
void launch_raygen(const RenderParams& rp, const BatchState& st, hipStream_t s);
void launch_shade_path(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int bounce,
                       int grid, hipStream_t s);
void launch_env(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int bounce, int grid, hipStream_t s);
void launch_shade_direct(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int stage,
                         int grid, hipStream_t s);
void launch_shade_spec(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int grid, hipStream_t s);
// dr_shade_whitted.hip: stage `stage` of a WhittedIntegrator vertex (light stage - 1 folded in, light `stage` set up)
void launch_shade_whitted(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int stage, int grid, hipStream_t s);
// dr_shade_ao.hip: one stage of AmbientOcclusionIntegrator.Li -- occlusion ray `fold` of every slot folded into its count (< 0: none), ray `emit` queued
// (< 0: none; 0: the camera hit set up first); the last ray folded: the slot's radiance nClear / nSamples
void launch_shade_ao(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, int nSamples, int fold, int emit,
                     double minDist, double maxDist, int grid, hipStream_t s);
// dr_shade_feature.hip: the one stage of the feature integrator -- channel DR_FEATURE_* of every slot's camera hit as its radiance (a miss: 0)
void launch_shade_feature(const DScene& sc, const BatchState& st, const StageQueues& q, int channel, int grid, hipStream_t s);
// dr_shade_material.hip: the one stage of the material integrator -- channel DR_MATERIAL_CHANNEL_* of every slot's camera ray as its radiance
void launch_shade_material(const DScene& sc, const BatchState& st, const StageQueues& q, int channel, int grid, hipStream_t s);
// dr_guides.hip (DESIGN.md 2.26): behind the camera rays' traversal, the DR_FEATURE_* channels of `mask` (bit = channel) of every slot's camera hit
// into the side planes of `side` ([3 * channels][sideCap] floats; a miss: 0); and, at the batch's film step, plane `plane` (the channel's rank in
// the mask) into the state's radiance plane, from where launch_film adds it to the channel's film
void launch_guides(const DScene& sc, const BatchState& st, float* side, uint32_t sideCap, uint32_t mask, TraceCounters* ctr, int grid, hipStream_t s);
void launch_guide_plane(const BatchState& st, const float* side, uint32_t sideCap, int plane, int grid, hipStream_t s);
void launch_film(const RenderParams& rp, const BatchState& st, const float* filterTable, uint32_t npix, float* film,
                 hipStream_t s);
void launch_film_resolve(const float* film, int64_t npix, float* rgb, hipStream_t s);
void launch_copy(const float4* src, float4* dst, uint64_t n4, hipStream_t s);
int layout_state_words();  // the layout this set of kernels was compiled for: DR_STATE_WORDS_K,
int layout_sub();          //   DR_SUB (LayoutOps in dr_api.hip reads and checks them)
void trace_prof_dump();  // -DDR_TRACE_PROF builds only: per-phase cycle sums of the v2 traversal loop
void shade_prof_dump();  // -DDR_SHADE_PROF builds only: prints and clears the per-phase cycle sums of k_shade_path

