// fp32 forward / data gradient: which kernel family a geometry gets, and the entry points behind capi.hip.
//
// FAMILIES is the one place the priority order is written.  Every question about a layer -- its kernel id, the size of
// its packed image, the packing, the statistics workspace, the run -- goes to the family that select() returns, so the
// plan that sizes an image or a workspace and the launch that uses it cannot disagree.  A new family: write its
// ConvFamily record next to its kernels, declare it in kernels.hpp, insert it here.
#include "common.hpp"
#include "kernels.hpp"

namespace {

// flat_t64 stands before flat_t4: under BP_FLATW_THIN both accept the 32 -> 16 k4 s2 transposed layer and t64 takes it.
// No earlier family can shadow either (enc, stem and flat want k8, k5 and k7).  The tiled kernels accept everything.
const ConvFamily& (*const FAMILIES[])() = {bp_family_enc,     bp_family_stem,    bp_family_flat,
                                          bp_family_flat_t64, bp_family_flat_t4, bp_family_flat_g4,
                                          bp_family_flat_h7,  bp_family_small,   bp_family_tiled};

const ConvFamily& select(const ConvGeom& g) {
  for (const auto family : FAMILIES)
    if (family().ok(g)) return family();
  return bp_family_tiled();
}

}  // namespace

int bp_igemm_kernel_id(const ConvGeom& g) { return select(g).kernel_id(g); }

int64_t bp_igemm_packed_floats(const ConvGeom& g) { return select(g).packed_floats(g); }

int bp_igemm_pack(const ConvGeom& g, const WeightMap& wm, const float* w_torch, float* packed, hipStream_t st) {
  return select(g).pack(g, wm, w_torch, packed, st);
}

int bp_igemm_pack_job(const ConvGeom& g, const WeightMap& wm, const float* w_torch, float* packed, void* job,
                      int64_t* nblocks) {
  if (!select(g).batched_pack) return BP_EUNSUPPORTED;       // (its own tiny pack kernel: packed by bp_conv_pack)
  return bp_igemm_tiled_pack_job(g, wm, w_torch, packed, job, nblocks);
}

size_t bp_igemm_stats_workspace(const ConvGeom& g, const bp_view* in, const bp_view* out, int mode) {
  return select(g).stats_workspace(g, in, out, mode);
}

int bp_igemm_run(const ConvGeom& g, const bp_view* in, const PW& pw, const float* packed, const float* bias,
                 const bp_view* out, hipStream_t st, const IgemmStatsReq* sr) {
  return select(g).run(g, in, pw, packed, bias, out, st, sr);
}
