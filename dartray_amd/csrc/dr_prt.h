// dr_prt.h -- what the diffuse PRT integrator's two units (dr_shade_prt.hip, dr_prt_project.hip) share with the host units.
// Included behind dr_kernels.h; kept out of dr_kernels.h / dr_launchers.inc, which the path, traversal and sampler kernels are compiled from.
#ifndef DR_PRT_H
#define DR_PRT_H

#include "dr_sh.h"

// k_shade_prt's own arguments: the rounded ray count, lmax, the render's side buffer c[Terms(lmax)][stride] of transfer coefficients, the table
// K[Terms(lmax)] of sh_K_table and the scene's incident-light coefficients c_in[Terms(lmax)][3]
struct PrtArgs {
  int32_t nSamples, lmax;
  uint32_t stride, pad;  // slots between two terms of c: the render's batch capacity (every slot of a batch is below it)
  float* c;
  const double* K;
  const float* cin;
};

// dr_shade_prt.hip: one stage of DiffusePRTIntegrator.Li -- occlusion ray `fold` of every slot folded into its transfer coefficients (< 0: none), ray
// `emit` queued (< 0: none; 0: the camera hit set up first); the last ray folded: L += Kd * clamp(c_in . c).  One copy per state layout.
void launch_shade_prt(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, const PrtArgs& a, int fold, int emit, int grid,
                      hipStream_t s);
namespace sp4 {
void launch_shade_prt(const DScene& sc, const RenderParams& rp, const BatchState& st, const StageQueues& q, const PrtArgs& a, int fold, int emit, int grid,
                      hipStream_t s);
}

struct DrScene;
namespace dr_host {
// dr_prt_project.hip: DiffusePRTIntegrator.preprocess on the device.  Leaves the scene's c_in for `lmax` in sc->prt.cin (computed once per scene and
// lmax) and the K table in sc->prt.K; waits for the stream.  lmax must have been checked (prtRefusal).
int prtIncident(DrScene* sc, int lmax, double shutterOpen, hipStream_t s);
// null, or why this lmax / nsamples is refused (DR_ERR_INVALID)
inline const char* prtRefusal(int32_t lmax, int32_t nsamples, bool checkSamples) {
  if (lmax < 1) return "diffuse PRT: lmax must be at least 1 (the Legendre recurrence stores P(1, 0) unconditionally)";
  if (lmax > DR_SH_LMAX_MAX) return "diffuse PRT: lmax above 8 (a camera sample's transfer coefficients, (lmax + 1)^2 words, live in a per-slot side buffer)";
  if (!checkSamples) return nullptr;
  if (nsamples < 1) return "diffuse PRT: nsamples must be at least 1";
  if (nsamples > 4096) return "diffuse PRT: nsamples above 4096 after rounding up to a power of two (the samplers' cap)";
  return nullptr;
}
}  // namespace dr_host

#endif
