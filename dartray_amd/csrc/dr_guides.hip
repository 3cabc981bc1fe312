// dr_guides.hip -- k_guides: the denoisers' guide images in the beauty render's own pass (dr_render_guides*).  Behind the
// camera stage's closest-hit traversal every slot still holds what k_shade_feature reads -- the hit record (F_HPRIM, F_HT) and the camera ray
// (F_RO, F_RD) -- and the integrator's first shading launch has not yet overwritten the ray.  One launch here, between the two, stores the value
// of every requested DR_FEATURE_* channel into that channel's SIDE PLANE; the batch's film step then, behind the beauty film, moves each plane
// into the state's radiance plane (k_guide_plane) and runs k_film, unchanged, into a film of the channel's own.
//
// One lane per slot, slots in order, like k_shade_feature.  A slot's loads and its hit geometry are done once and shared by the channels: hit_rec
// and hit_srec once, hit_dg once where ng, ns or a recorded triangle's uv asks for isect.dg, hit_dgs only where ns is requested.  The channel
// set is a kernel argument -- a bit per DR_FEATURE_* value -- uniform over the launch: every test of it is a scalar branch no wave diverges on,
// and one instantiation per state layout serves all 31 sets.  The values are dr_feature_value.h's, operator for operator those of
// k_shade_feature, so a plane holds the bytes the feature integrator's radiance plane would.
//
// Side planes: requested channel number k (in DR_FEATURE_* order) owns rows 3 k .. 3 k + 2 of side[3 * channels][sideCap]: component c of slot
// s at side[(3 k + c) * sideCap + s], a wave's store one 256-byte run.  k_guides writes nothing of the state: not F_L, not F_FLAGS, nor any
// other field a stage reads.  k_guide_plane writes F_L when the batch's stages are over and its beauty film has been added.  (k_film takes its
// radiance and its image samples off one base pointer, BatchState::tiles, and dr_kernels.h is pinned by the committed profiles: a plane cannot
// be handed to it as a view of the state, so it is moved to where k_film reads.)
// f64 arithmetic, one rounding to f32; compiled with -ffp-contract=off, like every unit.
#include "dr_kernels.h"
#include "dr_wave.h"

#ifdef DR_NS  // the second state layout (-DDR_SUB=4 -DDR_NS=sp4): every symbol in its own namespace
namespace DR_NS {
#endif

#include "dr_shade_common.h"
#include "dr_shade_hit.h"
#include "dr_shade_loop.h"
#include "dr_feature_value.h"

#define DR_GUIDES_BLOCK 256

// (slotBase: side + slot; cap: sideCap)
DR_DEV void guide_store(float* slotBase, size_t cap, uint32_t plane, C3 v) {
  float* p = slotBase + 3u * plane * cap;
  STS_STREAM(p, v.r);
  STS_STREAM(p + cap, v.g);
  STS_STREAM(p + 2 * cap, v.b);
}

__global__ void __launch_bounds__(DR_GUIDES_BLOCK) k_guides(DScene sc, BatchState st, float* side, uint32_t sideCap, uint32_t mask, TraceCounters* ctr) {
  __shared__ uint32_t s_hits;
  per_slot_begin(s_hits);
  const uint32_t stride = gridDim.x * blockDim.x;
  // the channel set and every channel's plane: uniform over the launch (scalar registers)
  const bool wNG = mask & (1u << DR_FEATURE_NG), wNS = mask & (1u << DR_FEATURE_NS), wD = mask & (1u << DR_FEATURE_DEPTH),
             wUV = mask & (1u << DR_FEATURE_UV), wID = mask & (1u << DR_FEATURE_ID);
  const uint32_t pNG = 0u, pNS = __popc(mask & ((1u << DR_FEATURE_NS) - 1u)), pD = __popc(mask & ((1u << DR_FEATURE_DEPTH) - 1u)),
                 pUV = __popc(mask & ((1u << DR_FEATURE_UV) - 1u)), pID = __popc(mask & ((1u << DR_FEATURE_ID) - 1u));
  const size_t cap = sideCap;
  uint32_t hits = 0u;
  for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < st.nslots; slot += stride) {
    const SlotRef sr = SlotRef::of(st, slot);
    float* out = side + slot;
    const int prim = sr.i32<F_HPRIM>();
    if (prim < 0) {  // the camera ray hit nothing: 0, 0, 0 in every plane
      const C3 zero = C3{0.f, 0.f, 0.f};
      if (wNG) guide_store(out, cap, pNG, zero);
      if (wNS) guide_store(out, cap, pNS, zero);
      if (wD) guide_store(out, cap, pD, zero);
      if (wUV) guide_store(out, cap, pUV, zero);
      if (wID) guide_store(out, cap, pID, zero);
      continue;
    }
    ++hits;
    const double t = sr.f64<F_HT>();
    if (wD) guide_store(out, cap, pD, feature_depth(t));
    if (wNG || wNS || wUV) {
      const HitRec h = hit_rec(sc, (uint32_t)prim);
      const ShadeRec srec = hit_srec(sc, h);
      const F3 o = ld3f<F_RO>(sr), d = ld3f<F_RD>(sr);
      DGeo dg = {};
      double u = 0.0, v = 0.0;
      const bool uvOwn = wUV && feature_uv_without_dg(sc, h, o, d, t, &u, &v);  // (a quadric, the default uvs: not isect.dg's)
      if (wNG || wNS || (wUV && !uvOwn)) {
        hit_dg(sc, h, srec, o, d, t, &dg);
        if (!uvOwn) {
          u = dg.u;
          v = dg.v;
        }
      }
      if (wNG) guide_store(out, cap, pNG, feature_normal(dg.nn));
      if (wNS) {
        DGeo dgs = {};
        hit_dgs(sc, h, srec, dg, &dgs);  // (a quadric's Shape.getShadingGeometry: a copy)
        guide_store(out, cap, pNS, feature_normal(dgs.nn));
      }
      if (wUV) guide_store(out, cap, pUV, feature_uv(u, v));
      if (wID) guide_store(out, cap, pID, feature_id(prim, h.tr.mat));
    } else if (wID) {
      guide_store(out, cap, pID, feature_id(prim, load_tri(sc, (uint32_t)prim).mat));
    }
  }
  per_slot_end(s_hits, hits, ctr, st.nslots);
}

// Plane `plane` into the radiance of every slot: the film step of one guide channel, in front of its k_film launch
__global__ void __launch_bounds__(DR_GUIDES_BLOCK) k_guide_plane(BatchState st, const float* side, uint32_t sideCap, uint32_t plane) {
  const uint32_t stride = gridDim.x * blockDim.x;
  const size_t cap = sideCap;
  for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < st.nslots; slot += stride) {
    const float* p = side + 3u * plane * cap + slot;
    stcf<F_L>(SlotRef::of(st, slot), C3{LDS_STREAM(p), LDS_STREAM(p + cap), LDS_STREAM(p + 2 * cap)});
  }
}

void launch_guides(const DScene& sc, const BatchState& st, float* side, uint32_t sideCap, uint32_t mask, TraceCounters* ctr, int grid, hipStream_t s) {
  // (BatchRunner::run holds the contract, loudly, before the batch's first launch: planes allocated, st.nslots <= sideCap)
  launch_per_slot<k_guides, DR_GUIDES_BLOCK>(grid, st.nslots, s, sc, st, side, sideCap, mask, ctr);
}

void launch_guide_plane(const BatchState& st, const float* side, uint32_t sideCap, int plane, int grid, hipStream_t s) {
  launch_per_slot<k_guide_plane, DR_GUIDES_BLOCK>(grid, st.nslots, s, st, side, sideCap, (uint32_t)plane);
}

#ifdef DR_NS
}  // namespace DR_NS
#endif
