// C ABI of the convolution entry points (include/bp_hip.h): shape validation on the host, then the dispatchers
// declared in kernels.hpp -- conv_dispatch.hip (fp32 forward / data gradient: one table of kernel families),
// conv_wgrad.hip (weight gradient), conv_bf16.hip (bf16) -- or the direct kernels of conv_direct.hip.
#include "common.hpp"
#include "kernels.hpp"
#include <cstring>

namespace {

bool conv_ok(const bp_conv* cv) {
  return cv && cv->cin > 0 && cv->cout > 0 && cv->k > 0 && cv->stride > 0 && cv->pad >= 0 && cv->out_pad >= 0 &&
         (cv->transposed == 0 || cv->transposed == 1) && (cv->transposed || cv->out_pad == 0) &&
         cv->out_pad < cv->stride + (cv->stride == 1);
}

// x: module input, y: module output (fp32 views unless `any`)
bool shapes_ok(const bp_conv* cv, const bp_view* x, const bp_view* y, bool any = false) {
  if (any ? (!bp_view_ok_any(x) || !bp_view_ok_any(y)) : (!bp_view_ok(x) || !bp_view_ok(y))) return false;
  if (x->n != y->n || x->c != cv->cin || y->c != cv->cout) return false;
  return y->h == bp_conv_out_extent(cv, x->h) && y->w == bp_conv_out_extent(cv, x->w) && y->h > 0 && y->w > 0;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

struct WgradPrivateWs {
  explicit WgradPrivateWs(bool on) { bp_wgrad_private_ws(on); }
  ~WgradPrivateWs() { bp_wgrad_private_ws(false); }
};

extern "C" {

int bp_version(void) { return 100; }

int bp_set_option(const char* name, int value) {
  if (!name) return BP_EINVAL;
  if (!strcmp(name, "bf16_ws")) { bp_bf16_ws_set(value); return BP_OK; }
  if (!strcmp(name, "f32_ws")) { bp_f32_ws_set(value); return BP_OK; }
  if (!strcmp(name, "f32_wgrad_ws")) { bp_f32_wgrad_ws_set(value); return BP_OK; }
  // (also under the name of the environment variable that sets its default)
  if (!strcmp(name, "bf16_wgrad_ws") || !strcmp(name, "BP_BF16_WGRAD_WS")) { bp_bf16_wgrad_ws_set(value); return BP_OK; }
  return BP_EUNSUPPORTED;
}

const char* bp_strerror(int code) {
  switch (code) {
    case BP_OK: return "ok";
    case BP_EINVAL: return "invalid argument (null pointer or inconsistent shapes)";
    case BP_EUNSUPPORTED: return "shape not supported by the gfx950 kernels";
    case BP_ELAUNCH: return "kernel launch failed";
    case BP_EWORKSPACE: return "workspace missing or too small";
  }
  return "unknown error";
}

int64_t bp_conv_packed_floats(const bp_conv* cv, int dir) {
  if (!conv_ok(cv) || (dir != BP_PACK_FWD && dir != BP_PACK_BWD)) return -1;
  const ConvGeom g = dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv);
  return bp_igemm_packed_floats(g);
}

int bp_conv_kernel_id(const bp_conv* cv, int dir) {
  if (!conv_ok(cv) || (dir != BP_PACK_FWD && dir != BP_PACK_BWD)) return -1;
  return bp_igemm_kernel_id(dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv));
}

int bp_conv_pack(const bp_conv* cv, int dir, const float* w_torch, float* packed, void* stream) {
  if (!conv_ok(cv) || !w_torch || !packed || (dir != BP_PACK_FWD && dir != BP_PACK_BWD)) return BP_EINVAL;
  const ConvGeom g = dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv);
  return bp_igemm_pack(g, bp_wmap(cv, dir), w_torch, packed, bp_stream(stream));
}

int32_t bp_conv_pack_job_bytes(void) { return (int32_t)bp_igemm_pack_job_bytes(); }

int bp_conv_pack_job(const bp_conv* cv, int dir, const float* w_torch, float* packed, void* job, int64_t* nblocks) {
  if (!conv_ok(cv) || !w_torch || !packed || !job || !nblocks || (dir != BP_PACK_FWD && dir != BP_PACK_BWD))
    return BP_EINVAL;
  const ConvGeom g = dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv);
  return bp_igemm_pack_job(g, bp_wmap(cv, dir), w_torch, packed, job, nblocks);
}

int bp_conv_pack_jobs(const void* jobs_dev, const int64_t* first_block_dev, int32_t njobs, int64_t total_blocks,
                      void* stream) {
  if (!jobs_dev || !first_block_dev || njobs < 0 || total_blocks < 0) return BP_EINVAL;
  return bp_igemm_pack_jobs(jobs_dev, first_block_dev, njobs, total_blocks, bp_stream(stream));
}

int64_t bp_conv_bf16_packed_elems(const bp_conv* cv, int dir) {
  if (!conv_ok(cv) || (dir != BP_PACK_FWD && dir != BP_PACK_BWD)) return -1;
  return bp_bf16_packed_elems(dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv));
}

int bp_conv_bf16_pack(const bp_conv* cv, int dir, const float* w_torch, void* packed, void* stream) {
  if (!conv_ok(cv) || !w_torch || !packed || (dir != BP_PACK_FWD && dir != BP_PACK_BWD)) return BP_EINVAL;
  const ConvGeom g = dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv);
  return bp_bf16_pack(g, bp_wmap(cv, dir), w_torch, packed, bp_stream(stream));
}

int bp_conv_ws_kind(const bp_conv* cv, int dir, const bp_view* in, const bp_view* out) {
  if (!conv_ok(cv) || (dir != BP_PACK_FWD && dir != BP_PACK_BWD) || !bp_view_ok_any(in) || !bp_view_ok_any(out)) return 0;
  const ConvGeom g = dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv);
  if (in->dtype == BP_F32 && out->dtype == BP_F32) return bp_f32_ws_ok(g, in, out, nullptr, 0) ? 3 : 0;
  return bp_bf16_ws_ok(g, in, out, nullptr, 0) ? bp_bf16_ws_kind(g) : 0;
}

int bp_conv_bf16_supported(const bp_conv* cv, int dir, const bp_view* in, const bp_view* out) {
  if (!conv_ok(cv) || (dir != BP_PACK_FWD && dir != BP_PACK_BWD)) return 0;
  if ((in && !bp_view_ok_any(in)) || (out && !bp_view_ok_any(out))) return 0;
  return bp_bf16_igemm_ok(dir == BP_PACK_FWD ? bp_geom_forward(cv) : bp_geom_backward_data(cv), in, out) ? 1 : 0;
}

int bp_conv_forward(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw, const float* packed_fwd,
                    const float* w_torch, const float* bias, const bp_view* y, int impl, void* stream) {
  if (!conv_ok(cv) || !shapes_ok(cv, x, y, impl == BP_IMPL_BF16)) return BP_EINVAL;
  const ConvGeom g = bp_geom_forward(cv);
  if (impl == BP_IMPL_BF16) {
    if (!packed_fwd) return BP_EINVAL;
    return bp_bf16_igemm_run(g, x, bp_pw(x_pw), packed_fwd, bias, y, bp_stream(stream));
  }
  if (impl == BP_IMPL_AUTO && packed_fwd) {
    // the register-resident kernels (conv_flat.hip) want 16-byte aligned produced views: AUTO takes the direct kernel
    // for the odd view instead of refusing it (BP_IMPL_MFMA, asked for by name, still reports BP_EUNSUPPORTED)
    const int rc = bp_igemm_run(g, x, bp_pw(x_pw), packed_fwd, bias, y, bp_stream(stream));
    if (rc != BP_EUNSUPPORTED || !w_torch) return rc;
    impl = BP_IMPL_DIRECT;
  }
  if (impl == BP_IMPL_AUTO) impl = BP_IMPL_DIRECT;
  if (impl == BP_IMPL_MFMA) {
    if (!packed_fwd) return BP_EINVAL;
    return bp_igemm_run(g, x, bp_pw(x_pw), packed_fwd, bias, y, bp_stream(stream));
  }
  if (!w_torch) return BP_EINVAL;
  return bp_direct_gather(g, bp_wmap(cv, BP_PACK_FWD), x, bp_pw(x_pw), w_torch, bias, y, bp_stream(stream));
}

size_t bp_conv_stats_workspace(const bp_conv* cv, int dir, const bp_view* x, const bp_view* y, int impl) {
  if (!conv_ok(cv) || !shapes_ok(cv, x, y, impl == BP_IMPL_BF16) || (dir != BP_PACK_FWD && dir != BP_PACK_BWD)) return 0;
  if (impl == BP_IMPL_BF16)
    return dir == BP_PACK_FWD ? bp_bf16_stats_workspace(bp_geom_forward(cv), x, y, 1)
                              : bp_bf16_stats_workspace(bp_geom_backward_data(cv), y, x, 2);
  return dir == BP_PACK_FWD ? bp_igemm_stats_workspace(bp_geom_forward(cv), x, y, 1)
                            : bp_igemm_stats_workspace(bp_geom_backward_data(cv), y, x, 2);
}

int bp_conv_forward_stats(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw, const float* packed_fwd,
                          const bp_view* y, double* sums, void* workspace, size_t workspace_bytes, int impl,
                          void* stream) {
  if (!conv_ok(cv) || !shapes_ok(cv, x, y, impl == BP_IMPL_BF16) || !packed_fwd || !sums) return BP_EINVAL;
  const IgemmStatsReq sr{1, nullptr, PW{nullptr, nullptr, nullptr}, sums, workspace, workspace_bytes};
  if (impl == BP_IMPL_BF16)
    return bp_bf16_igemm_run(bp_geom_forward(cv), x, bp_pw(x_pw), packed_fwd, nullptr, y, bp_stream(stream), &sr);
  return bp_igemm_run(bp_geom_forward(cv), x, bp_pw(x_pw), packed_fwd, nullptr, y, bp_stream(stream), &sr);
}

int bp_conv_forward_bn(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw, const float* packed_fwd,
                       const bp_view* y, double* sums, const bp_bn_train* bn, void* workspace, size_t workspace_bytes,
                       int impl, void* stream) {
  if (!conv_ok(cv) || !shapes_ok(cv, x, y, impl == BP_IMPL_BF16) || !packed_fwd || !sums || !bn || bn->count <= 0 ||
      !bn->scale || !bn->shift)
    return BP_EINVAL;
  const BnFin fin{bn->count, bn->gamma, bn->beta, bn->eps, bn->momentum, bn->running_mean, bn->running_var,
                  bn->num_batches_tracked, bn->scale, bn->shift, bn->save_mean, bn->save_invstd};
  const IgemmStatsReq sr{1, nullptr, PW{nullptr, nullptr, nullptr}, sums, workspace, workspace_bytes, &fin};
  if (impl == BP_IMPL_BF16)
    return bp_bf16_igemm_run(bp_geom_forward(cv), x, bp_pw(x_pw), packed_fwd, nullptr, y, bp_stream(stream), &sr);
  return bp_igemm_run(bp_geom_forward(cv), x, bp_pw(x_pw), packed_fwd, nullptr, y, bp_stream(stream), &sr);
}

int bp_conv_backward_data_stats(const bp_conv* cv, const bp_view* dy, const float* packed_bwd, const bp_view* dx,
                                const bp_view* x_raw, const bp_pointwise* x_pw, double* sums, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const bool b16 = (dy && dy->dtype == BP_BF16) || (dx && dx->dtype == BP_BF16);        // the bf16 kernels' epilogue
  if (!conv_ok(cv) || !shapes_ok(cv, dx, dy, b16) || !packed_bwd || !sums || !bp_view_ok_any(x_raw)) return BP_EINVAL;
  if (x_raw->n != dx->n || x_raw->h != dx->h || x_raw->w != dx->w || x_raw->c != dx->c) return BP_EINVAL;
  const IgemmStatsReq sr{2, x_raw, bp_pw(x_pw), sums, workspace, workspace_bytes};
  if (b16)
    return bp_bf16_igemm_run(bp_geom_backward_data(cv), dy, PW{nullptr, nullptr, nullptr}, packed_bwd, nullptr, dx,
                             bp_stream(stream), &sr);
  if (!bp_view_ok(x_raw)) return BP_EINVAL;
  return bp_igemm_run(bp_geom_backward_data(cv), dy, PW{nullptr, nullptr, nullptr}, packed_bwd, nullptr, dx,
                      bp_stream(stream), &sr);
}

size_t bp_conv_backward_data_act_workspace(const bp_conv* cv, const bp_view* dy, const bp_view* g) {
  const bool b16 = g && g->dtype == BP_BF16;              // the bf16 kernel's epilogue (conv_bf16_head.hip)
  if (!conv_ok(cv) || !shapes_ok(cv, g, dy, b16)) return 0;
  if (b16) return bp_bf16_stats_workspace(bp_geom_backward_data(cv), dy, g, 3);
  return bp_igemm_stats_workspace(bp_geom_backward_data(cv), dy, g, 3);
}

int bp_conv_backward_data_act(const bp_conv* cv, const bp_view* dy, const float* packed_bwd, const bp_view* g,
                              const bp_view* x_raw, const bp_pointwise* x_pw, double* sums, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const bool b16 = g && g->dtype == BP_BF16;
  if (!conv_ok(cv) || !shapes_ok(cv, g, dy, b16) || !packed_bwd || !sums || !bp_view_ok_any(x_raw)) return BP_EINVAL;
  if (x_raw->n != g->n || x_raw->h != g->h || x_raw->w != g->w || x_raw->c != g->c) return BP_EINVAL;
  const IgemmStatsReq sr{3, x_raw, bp_pw(x_pw), sums, workspace, workspace_bytes};
  if (b16) {
    // (only the head kernel has this epilogue: the generic bf16 kernel would ignore the request)
    const ConvGeom gm = bp_geom_backward_data(cv);
    if (!bp_bf16_stats_workspace(gm, dy, g, 3)) return BP_EUNSUPPORTED;
    return bp_bf16_igemm_run(gm, dy, PW{nullptr, nullptr, nullptr}, packed_bwd, nullptr, g, bp_stream(stream), &sr);
  }
  if (!bp_view_ok(x_raw)) return BP_EINVAL;
  return bp_igemm_run(bp_geom_backward_data(cv), dy, PW{nullptr, nullptr, nullptr}, packed_bwd, nullptr, g,
                      bp_stream(stream), &sr);
}

int bp_conv_backward_data(const bp_conv* cv, const bp_view* dy, const float* packed_bwd, const float* w_torch,
                          const bp_view* dx, int impl, void* stream) {
  if (!conv_ok(cv) || !shapes_ok(cv, dx, dy, impl == BP_IMPL_BF16)) return BP_EINVAL;
  const ConvGeom g = bp_geom_backward_data(cv);
  if (impl == BP_IMPL_BF16) {
    if (!packed_bwd) return BP_EINVAL;
    return bp_bf16_igemm_run(g, dy, PW{nullptr, nullptr, nullptr}, packed_bwd, nullptr, dx, bp_stream(stream));
  }
  if (impl == BP_IMPL_AUTO && packed_bwd) {
    const int rc = bp_igemm_run(g, dy, PW{nullptr, nullptr, nullptr}, packed_bwd, nullptr, dx, bp_stream(stream));
    if (rc != BP_EUNSUPPORTED || !w_torch) return rc;
    impl = BP_IMPL_DIRECT;
  }
  if (impl == BP_IMPL_AUTO) impl = BP_IMPL_DIRECT;
  if (impl == BP_IMPL_MFMA) {
    if (!packed_bwd) return BP_EINVAL;
    return bp_igemm_run(g, dy, PW{nullptr, nullptr, nullptr}, packed_bwd, nullptr, dx, bp_stream(stream));
  }
  if (!w_torch) return BP_EINVAL;
  return bp_direct_gather(g, bp_wmap(cv, BP_PACK_BWD), dy, PW{nullptr, nullptr, nullptr}, w_torch, nullptr, dx,
                          bp_stream(stream));
}

// The workspace of one layer: main, then the channel sums of dy, then 2 * c doubles.  `main_f32`: what the fp32 table
// asks for the layer's workspace query (0: fp32 not asked, or unsupported); the bf16 table's need is taken in as well,
// since the caller sizes one workspace per layer.
static size_t weight_workspace(const WgradCall& query, size_t main_f32, const bp_view* dy) {
  WgradSelection b;
  const size_t main_bf16 = bp_wgrad_select(true, query, &b) == BP_OK ? b.ws_bytes : 0;
  return align256(main_f32 > main_bf16 ? main_f32 : main_bf16) + align256(bp_channel_sums_workspace(dy)) +
         align256((size_t)2 * dy->c * sizeof(double));
}

// (a workspace query: no pointwise operand, un-shared)
static WgradCall weight_query(const bp_conv* cv, const bp_view* x, const bp_view* dy) {
  const PW none{nullptr, nullptr, nullptr};
  return WgradCall{cv, cv->transposed ? dy : x, none, cv->transposed ? x : dy, none, false};
}

size_t bp_conv_backward_weight_workspace(const bp_conv* cv, const bp_view* x, const bp_view* dy) {
  if (!conv_ok(cv) || !shapes_ok(cv, x, dy, true)) return 0;
  const WgradCall query = weight_query(cv, x, dy);
  WgradSelection f;
  const bool f32 = x->dtype == BP_F32 && dy->dtype == BP_F32 && bp_wgrad_select(false, query, &f) == BP_OK;
  return weight_workspace(query, f32 ? f.ws_bytes : 0, dy);
}

// The call and bp_conv_backward_weight_plan (`plan`: nothing is launched, no workspace is asked for; plan = {family,
// nsplit, cxp, cyp} of the kernel the call would run).  The table is walked once for the layer's workspace query; that
// selection is the call's own unless the call carries what the query does not (a pointwise operand, BP_IMPL_SHARED),
// and then the table is walked once more for the call.
static int backward_weight(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw, const bp_view* dy,
                           float* dw_torch, float* dbias, void* workspace, size_t workspace_bytes, int impl,
                           void* stream, int32_t* plan) {
  const bool shared = (impl & BP_IMPL_SHARED) != 0;
  const WgradPrivateWs priv(!plan && (impl & BP_IMPL_DEFER) != 0);      // (this call's reduction may wait for the flush)
  impl &= ~(BP_IMPL_SHARED | BP_IMPL_DEFER);
  if (!conv_ok(cv) || !shapes_ok(cv, x, dy, impl == BP_IMPL_BF16) || (!plan && !dw_torch)) return BP_EINVAL;
  const bool bf16 = impl == BP_IMPL_BF16;
  const WgradCall query = weight_query(cv, x, dy);
  WgradCall call = query;
  (cv->transposed ? call.pwy : call.pwx) = bp_pw(x_pw);
  call.shared = shared && !bf16;             // (the bf16 kernels have no shared form)
  hipStream_t st = bp_stream(stream);
  if (bf16 && dbias) return BP_EUNSUPPORTED;       // (bias gradients: the fp32 path; the CVAE's convolutions have none)
  WgradSelection sel;
  const bool found = bp_wgrad_select(bf16, query, &sel) == BP_OK;
  if (bf16 && !found) return BP_EUNSUPPORTED;
  size_t ws_main = bf16 ? workspace_bytes : 0;      // bytes of `workspace` the kernel may use
  if (bf16) {
    if (!plan && (!workspace || workspace_bytes < sel.ws_bytes)) return BP_EWORKSPACE;
  } else {
    ws_main = found ? align256(sel.ws_bytes) : 0;
    if (impl == BP_IMPL_AUTO) impl = found ? BP_IMPL_MFMA : BP_IMPL_DIRECT;
    if (!plan && (impl == BP_IMPL_MFMA || dbias)) {
      if (!workspace || workspace_bytes < weight_workspace(query, found ? sel.ws_bytes : 0, dy)) return BP_EWORKSPACE;
    }
    if (impl == BP_IMPL_MFMA && !found) return BP_EUNSUPPORTED;
  }
  int rc;
  if (bf16 || impl == BP_IMPL_MFMA) {
    if ((call.pwx.scale || call.pwy.scale || call.shared) && bp_wgrad_select(bf16, call, &sel) != BP_OK)
      return BP_EUNSUPPORTED;
    if (plan) {
      plan[0] = sel.row.id; plan[1] = sel.row.nsplit; plan[2] = sel.row.cxp; plan[3] = sel.row.cyp;
      return BP_OK;
    }
    rc = bp_wgrad_run(sel, call, dw_torch, workspace, ws_main, st);
  } else if (plan) {
    plan[0] = BP_WG_DIRECT; plan[1] = plan[2] = plan[3] = 0;
    rc = BP_OK;
  } else {
    rc = bp_direct_wgrad(cv, call.X, call.pwx, call.Y, call.pwy, dw_torch, st);
  }
  if (rc != BP_OK || plan) return rc;
  if (dbias) {
    char* base = reinterpret_cast<char*>(workspace) + ws_main;
    const size_t ws_sums = align256(bp_channel_sums_workspace(dy));
    double* sums = reinterpret_cast<double*>(base + ws_sums);
    rc = bp_channel_sums(dy, sums, base, ws_sums, stream);
    if (rc != BP_OK) return rc;
    rc = bp_sums_to_float(sums, dy->c, dbias, stream);
  }
  return rc;
}

int bp_conv_backward_weight(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw, const bp_view* dy,
                            float* dw_torch, float* dbias, void* workspace, size_t workspace_bytes, int impl,
                            void* stream) {
  return backward_weight(cv, x, x_pw, dy, dw_torch, dbias, workspace, workspace_bytes, impl, stream, nullptr);
}

int bp_conv_backward_weight_plan(const bp_conv* cv, const bp_view* x, const bp_view* dy, int impl, int32_t out[4]) {
  if (!out) return BP_EINVAL;
  out[0] = -1; out[1] = out[2] = out[3] = 0;
  const int rc = backward_weight(cv, x, nullptr, dy, nullptr, nullptr, nullptr, 0, impl, nullptr, out);
  if (rc != BP_OK) { out[0] = -1; out[1] = out[2] = out[3] = 0; }
  return rc;
}

int bp_wgrad_defer_begin(void) { return bp_wgrad_defer_begin_impl(); }
int bp_wgrad_defer_flush(int end, void* stream) { return bp_wgrad_defer_flush_impl(bp_stream(stream), end); }

}  // extern "C"
