// dr_gprt.h -- what the glossy PRT integrator's units (dr_shade_gprt.hip, dr_prt_project.hip) share with the host units.
// Included behind dr_kernels.h and dr_prt.h; kept out of dr_kernels.h / dr_launchers.inc like dr_prt.h.
#ifndef DR_GPRT_H
#define DR_GPRT_H

#include "dr_sh_glossy.h"

// k_shade_gprt's and k_gprt_finish's arguments: the rounded ray count, lmax, the render's side buffers -- bits[words][stride], one visibility bit
// per ray and slot (words = max(1, nSamples / 32)), and mark[stride], 1 for a slot whose camera ray hit -- the table K of sh_K_table, the scene's
// incident-light coefficients c_in[Terms][3] and the BSDF matrix B[Terms][Terms][3]
struct GprtArgs {
  int32_t nSamples, lmax;
  uint32_t stride, words;  // slots between two words of bits: the render's batch capacity (every slot of a batch is below it)
  uint32_t* bits;
  uint32_t* mark;
  const double* K;
  const float* cin;
  const float* B;
};

// dr_shade_gprt.hip: one stage of GlossyPRTIntegrator.Li's ComputeTransferMatrix -- the visibility of occlusion ray `fold` of every slot recorded
// (< 0: none), ray `emit` queued (< 0: none; 0: the camera hit set up first) -- and, once per batch behind the last fold, the rest of Li: one
// wave per slot.  One copy per state layout.
void launch_shade_gprt(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, const GprtArgs& a, int fold, int emit, int grid,
                       hipStream_t s);
void launch_gprt_finish(const BatchState& st, const GprtArgs& a, hipStream_t s);
namespace sp4 {
void launch_shade_gprt(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, const GprtArgs& a, int fold, int emit, int grid,
                       hipStream_t s);
void launch_gprt_finish(const BatchState& st, const GprtArgs& a, hipStream_t s);
}

struct DrScene;
namespace dr_host {
// dr_prt_project.hip: ComputeBSDFMatrix (core/spherical_harmonics.dart:609-672) on the device for the scene's glossy parameters, nsamples_b
// directions; leaves B[Terms][Terms][3] in sc->gprt.B (computed once per (lmax, nsamples_b, Kd, Ks, roughness)); waits for the stream.  Calls
// prtIncident first: the scramble is the two draws that follow whatever the light projection consumed.
int gprtBsdfMatrix(DrScene* sc, int lmax, int nsamples_b, double shutterOpen, hipStream_t s);
// one lane of the device runs sh_rotate_channel per channel and frame (dr_sh_rotate_device)
int gprtRotateDevice(const float* c_in, const float* m16, int lmax, int nframes, float* out);
// null, or why this lmax / nsamples is refused (DR_ERR_INVALID)
inline const char* gprtRefusal(int32_t lmax, int32_t nsamples, bool checkSamples) {
  if (lmax < 1) return "glossy PRT: lmax must be at least 1 (the Legendre recurrence stores P(1, 0) unconditionally)";
  if (lmax > DR_GPRT_LMAX_MAX) return "glossy PRT: lmax above 4 (the x-rotation rows are restated band by band, and a wave's registers hold the 325 distinct elements of a transfer matrix at lmax 4)";
  if (!checkSamples) return nullptr;
  if (nsamples < 1) return "glossy PRT: nsamples must be at least 1";
  if (nsamples > 4096) return "glossy PRT: nsamples above 4096 after rounding up to a power of two (the samplers' cap)";
  return nullptr;
}
}  // namespace dr_host

#endif
