// dr_probes.h -- what the radiance-probe units (dr_shade_probes.hip, dr_probes.hip) share with the host units.
// Included behind dr_kernels.h and dr_prt.h; kept out of dr_kernels.h / dr_launchers.inc like dr_prt.h.
#ifndef DR_PROBES_H
#define DR_PROBES_H

#include "dr_sh.h"

// k_shade_probes' own arguments: the grid of UseProbesIntegrator (use_probes_integrator.dart:41-67) -- lmax, nProbes, the bounds, the
// coefficients c_in[cell][Terms(lmax)][3] -- and the table K of sh_K_table
struct ProbeArgs {
  int32_t lmax, n[3];
  float bmin[3], bmax[3];
  const float* cin;
  const double* K;
};

// dr_shade_probes.hip: UseProbesIntegrator.Li of every slot of the batch, one launch behind the camera rays' traversal; queues nothing.  One copy
// per state layout.
void launch_shade_probes(const DScene& sc, const BatchState& st, const StageQueues& q, const ProbeArgs& a, int grid, hipStream_t s);
namespace sp4 {
void launch_shade_probes(const DScene& sc, const BatchState& st, const StageQueues& q, const ProbeArgs& a, int grid, hipStream_t s);
}

namespace dr_host {
// The header of a probe file against its length (dr_scene_set_probes): null, or why it is refused (DR_ERR_INVALID).  n: floats.
inline const char* probesHeaderRefusal(const float* data, int64_t n) {
  if (n < 15) return "use probes: a probe grid has at least 15 floats (lmax, two flags, nProbes[3], six bounds, three trailing zeros)";
  for (int i = 0; i < 12; ++i)
    if (!(data[i] == data[i]) || data[i] - data[i] != 0.f) return "use probes: the grid's header holds a value that is not finite";
  const int lmax = (int)data[0];
  if (lmax < 1 || lmax > DR_SH_LMAX_MAX) return "use probes: lmax of the grid is outside 1 .. 8";
  int64_t cells = 1;
  for (int i = 3; i < 6; ++i) {
    if (!(data[i] >= 1.f) || data[i] > 4096.f || data[i] != (float)(int)data[i]) return "use probes: nProbes of the grid must be whole numbers in 1 .. 4096";
    cells *= (int64_t)data[i];
  }
  if (n != 15 + cells * sh_terms(lmax) * 3) return "use probes: the grid's length is not 15 + nProbes[0] * nProbes[1] * nProbes[2] * (lmax + 1)^2 * 3 floats";
  return nullptr;
}
}  // namespace dr_host

#endif
