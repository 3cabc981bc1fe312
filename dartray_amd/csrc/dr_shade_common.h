// dr_shade_common.h -- what a shading unit outside dr_kernels.hip needs of that file's own helpers: the launch shape, the LDS copy of
// the light tables, the vertex statistics and the launcher.  RESTATED from dr_kernels.hip word for word (shade_count, the DR_SHADE_* /
// DR_LDS_* macros, light_table_bytes, mat_table_bytes, stage_lights, launch_shade, lightsInLds), not moved: the committed round-6
// profiles carry the hash of dr_kernels.hip (tests/test_bench_line.py), so that file changes only together with new profiling passes.
// When it next does, it should include this header and drop its copies, and take the helpers that the units share among themselves --
// dr_shade_hit.h (the hit's geometry, isect.Le, the ray epsilon, the escaped ray, Spectrum.clamp), dr_shade_loop.h (the queue-fed stage
// loop, the one-lane-per-slot epilogue and launcher) and the scramble words of dr_li_sampling.h -- in place of the copies it holds inline
// in k_shade_path, k_shade_direct and k_shade_spec.  Only restated text belongs here (tests/test_whitted_integrator.py holds every block
// against dr_kernels.hip).  Used by the six dr_shade_*.hip units.
// Included INSIDE the unit's layout namespace (DR_NS), behind dr_kernels.h and dr_wave.h: includes nothing itself.
#ifndef DR_SHADE_COMMON_H
#define DR_SHADE_COMMON_H

// DrRenderStats.shade_items / shade_vertices: the per-wave vertex counts stage_push kept in LDS, one no-return atomic
// per workgroup at the end of a shade kernel
DR_DEV void shade_count(PushStage& sm, TraceCounters* ctr, uint32_t nIn) {
  if (threadIdx.x == 0) {
    unsigned long long v = 0;
    for (int w = 0; w < 16; ++w) v += sm.nVert[w];
    if (v) atomicAdd(&ctr->shade_vertices, v);
    if (blockIdx.x == 0) atomicAdd(&ctr->shade_items, (unsigned long long)nIn);
  }
}

// One vertex of PathIntegrator.Li (path_integrator.dart:44-119).
// Launch shape (measured, MEASUREMENTS.md): ONE 768-thread workgroup per CU = 3 waves per SIMD (168 VGPRs each);
// the waves are independent of each other (own staging region, own reservations, work taken in chunks), 4 waves per
// SIMD spill.
#ifndef DR_SHADE_WAVES
#define DR_SHADE_WAVES 3
#endif
#ifndef DR_SHADE_BLOCK
#define DR_SHADE_BLOCK 768
#endif
#ifndef DR_SHADE_GRID_PER_CU
#define DR_SHADE_GRID_PER_CU 1
#endif
#define DR_SHADE_GRID(numCU) ((numCU) * DR_SHADE_GRID_PER_CU)
// the general-material variants need more registers (188+ spilled VGPRs even at 2 waves per SIMD): 512 threads x 2
// waves per SIMD is ~20 % faster for them; the env-map path variant fits 3 waves once its env-map functions are
// called out of line (env_*_ni in dr_device.h)
#ifndef DR_SHADE_BLOCK_GEN
#define DR_SHADE_BLOCK_GEN 512
#endif
#ifndef DR_SHADE_WAVES_GEN
#define DR_SHADE_WAVES_GEN 2
#endif
#define SHADE_BLOCK_OF(general) ((general) ? DR_SHADE_BLOCK_GEN : DR_SHADE_BLOCK)
#define SHADE_WAVES_OF(general) ((general) ? DR_SHADE_WAVES_GEN : DR_SHADE_WAVES)
// LDS copy of the light tables and (when it is small too) the material table, behind the queue-staging block of the
// dynamic LDS; a workgroup-wide copy + barrier.
// Which tables go where at what sizes, and the test on either side of each cap: DESIGN.md section 3, "Where the tables live" (what
// dr_device.h sums up as "large emissive meshes keep the global tables"; that file's hash is pinned by the committed profiles).
#define DR_LDS_LIGHT_BYTES (24 * 1024)  // light tables up to this size are staged in LDS (the queue staging takes ~96 KB of the 160)
#define DR_LDS_MAT_BYTES (24 * 1024)    // likewise the material table (64 B per material)
__host__ __device__ inline size_t light_table_bytes(const DScene& sc) {  // (+ 48 B per triangle: its f64 edges, LdsLights::ledges)
  return (size_t)sc.nlights * sizeof(DLight) + (size_t)sc.nltris * (sizeof(DLightTri) + 48) + (size_t)sc.ncdf * 4;
}
__host__ __device__ inline size_t mat_table_bytes(const DScene& sc) {
  const size_t b = (size_t)sc.nmats * 64;
  return b <= DR_LDS_MAT_BYTES ? b : 0;
}
DR_DEV LdsLights stage_lights(const DScene& sc, unsigned char* dyn, size_t pushBytes) {
  uint32_t* dst = (uint32_t*)(dyn + pushBytes);
  const uint32_t nL = sc.nlights * (uint32_t)(sizeof(DLight) / 4), nT = sc.nltris * (uint32_t)(sizeof(DLightTri) / 4), nC = sc.ncdf;
  const uint32_t nE = sc.nltris * 12u;  // f64 edges; nL and nT are even (8-byte multiples), so they start 8-byte aligned
  const uint32_t nM = (uint32_t)(mat_table_bytes(sc) / 4);
  const uint32_t* srcL = (const uint32_t*)sc.lights;
  const uint32_t* srcT = (const uint32_t*)sc.ltris;
  const uint32_t* srcC = (const uint32_t*)sc.lcdf;
  const uint32_t* srcM = (const uint32_t*)sc.mats;
  for (uint32_t i = threadIdx.x; i < nL; i += blockDim.x) dst[i] = srcL[i];
  for (uint32_t i = threadIdx.x; i < nT; i += blockDim.x) dst[nL + i] = srcT[i];
  for (uint32_t i = threadIdx.x; i < sc.nltris * 6u; i += blockDim.x) {
    // e1 = p2 - p1, e2 = p3 - p1 as Triangle.intersect forms them (triangle.dart:52-57): f64 differences of f32 values
    const uint32_t t = i / 6u, k = i % 6u;
    const float* p = sc.ltris[t].p;
    const double e = (double)p[3 + k] - (double)p[k % 3u];
    dst[nL + nT + 2u * i] = (uint32_t)__double2loint(e);
    dst[nL + nT + 2u * i + 1u] = (uint32_t)__double2hiint(e);
  }
  for (uint32_t i = threadIdx.x; i < nC; i += blockDim.x) dst[nL + nT + nE + i] = srcC[i];
  for (uint32_t i = threadIdx.x; i < nM; i += blockDim.x) dst[nL + nT + nE + nC + i] = srcM[i];
  __syncthreads();
  LdsLights lv;
  lv.lights = (lds_cu32*)dst;
  lv.ltris = (lds_cu32*)(dst + nL);
  lv.ledges = (lds_cu32*)(dst + nL + nT);
  lv.lcdf = (lds_cu32*)(dst + nL + nT + nE);
  lv.mats = nM ? (lds_cu32*)(dst + nL + nT + nE + nC) : (lds_cu32*)nullptr;
  lv.gmats = sc.mats;
  return lv;
}

// The shade kernels stage their queue entries in dynamic LDS (PushStage, dr_wave.h): ~96 KB of the CU's 160 KB; the
// light tables follow when they are small (LLDS instantiations).
template <auto kernel, int BLOCK, int NQ = 4, class... A>
static void launch_shade(int grid, size_t extraLds, hipStream_t s, A... args) {
  const size_t lds = push_stage_bytes(BLOCK, NQ) + extraLds;
  static size_t attrSet = 0;  // one instance of this template, hence one value, per kernel
  if (attrSet < lds) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attrSet = lds;
  }
  hipLaunchKernelGGL(kernel, dim3(DR_SHADE_GRID(grid)), dim3(BLOCK), lds, s, args...);
}
static bool lightsInLds(const DScene& sc) {
  return sc.nlights > 0 && light_table_bytes(sc) <= DR_LDS_LIGHT_BYTES;
}

#endif
