// Every host function that crosses a translation unit, declared once and grouped by the file that defines it, and the
// records through which the dispatchers reach the kernel families: ConvFamily (forward / data gradient; the order is
// FAMILIES in conv_dispatch.hip) and WgradFamily (weight gradient; the order is F32_FAMILIES and BF16_FAMILIES in
// conv_wgrad.hip).  A new family: write its record next to its kernels, declare its accessor here, insert it into the
// table.  Include after common.hpp.  Default arguments live here only.
#pragma once
#include "common.hpp"

// ---- fp32 forward / data gradient: one record per kernel family (conv_dispatch.hip walks them in priority order).
// A family answers six questions about a geometry it accepts; the adapters that give its kernels' own entry points
// these signatures sit next to the kernels.
struct ConvFamily {
  const char* name;
  bool (*ok)(const ConvGeom& g);
  int (*kernel_id)(const ConvGeom& g);
  int64_t (*packed_floats)(const ConvGeom& g);
  int (*pack)(const ConvGeom& g, const WeightMap& wm, const float* w_torch, float* packed, hipStream_t st);
  // 0: this layer's kernel has no epilogue for `mode` (IgemmStatsReq) on these views
  size_t (*stats_workspace)(const ConvGeom& g, const bp_view* in, const bp_view* out, int mode);
  int (*run)(const ConvGeom& g, const bp_view* in, const PW& pw, const float* packed, const float* bias,
             const bp_view* out, hipStream_t st, const IgemmStatsReq* sr);
  bool batched_pack;      // bp_conv_pack_job may take it (false: its own tiny pack kernel, packed by bp_conv_pack)
};
// (Each record is a function-local static const behind an accessor: a const variable at namespace scope would be emitted
// into the device code object as well, where the host functions it points to do not exist.)
// adapters most families share: one kernel id; statistics of the produced tensor (mode 1) only
template <int ID>
int bp_family_id(const ConvGeom&) { return ID; }
template <size_t (*WS)(const bp_view* out)>
size_t bp_family_stats_mode1(const ConvGeom&, const bp_view*, const bp_view* out, int mode) { return mode == 1 ? WS(out) : 0; }

// conv_enc.hip: the k8 stride-4 layer 8 -> 16 of the recognition / prior networks, forward and data gradient, and k4 s2
// {1, 2} -> 8
const ConvFamily& bp_family_enc();
// conv_stem.hip: the 3 -> 16 k5 stem (flattened (tap column, channel) K, weights in registers)
const ConvFamily& bp_family_stem();
// conv_flat.hip: unit-stride k7, 8 gathered -> 16 produced channels (weights in registers, flattened K)
const ConvFamily& bp_family_flat();
// ... the stride-2 k4 transposed form 64 -> 32 (eight waves: four phases x two blocks of 16 produced channels)
const ConvFamily& bp_family_flat_t64();
// ... the stride-2 k4 transposed form 32 -> 16 (four phases, all weights in registers)
const ConvFamily& bp_family_flat_t4();
// ... the stride-2 k4 conv form 32 -> 64 (eight waves: four blocks of 16 produced channels, weights in registers)
const ConvFamily& bp_family_flat_g4();
// ... and unit-stride k7 16 -> 8 (the head's first layer forward: K split over two waves, pixel pairs per MFMA column)
const ConvFamily& bp_family_flat_h7();
// conv_small.hip: vector-ALU kernel for unit-stride layers with cin*cout <= 8, and the one-channel strided kernels
const ConvFamily& bp_family_small();
// conv_igemm.hip: the tiled implicit-GEMM kernels (takes every geometry: it refuses the ones it has no configuration
// for) and, by views, their hand-off to the weights-stationary kernel of conv_ws_f32.hip
const ConvFamily& bp_family_tiled();

// conv_dispatch.hip: the fp32 gather entry points behind capi.hip
int64_t bp_igemm_packed_floats(const ConvGeom& g);
int bp_igemm_kernel_id(const ConvGeom& g);
int bp_igemm_pack(const ConvGeom& g, const WeightMap& wm, const float* w_torch, float* packed, hipStream_t st);
int bp_igemm_pack_job(const ConvGeom& g, const WeightMap& wm, const float* w_torch, float* packed, void* job,
                      int64_t* nblocks);
int bp_igemm_run(const ConvGeom& g, const bp_view* in, const PW& pw, const float* packed, const float* bias,
                 const bp_view* out, hipStream_t st, const IgemmStatsReq* stats = nullptr);
size_t bp_igemm_stats_workspace(const ConvGeom& g, const bp_view* in, const bp_view* out, int mode);

// conv_igemm.hip: batched packing of the tiled kernels' images (the job record is the pack kernel's argument block)
size_t bp_igemm_pack_job_bytes();
int bp_igemm_tiled_pack_job(const ConvGeom& g, const WeightMap& wm, const float* w_torch, float* packed, void* job,
                            int64_t* nblocks);
int bp_igemm_pack_jobs(const void* jobs_dev, const int64_t* first_block_dev, int njobs, int64_t total_blocks,
                       hipStream_t st);
// conv_igemm.hip: partial rows [rows][2*C] of epilogue statistics -> sr->sums (bytes of workspace for the rows and their
// first fold, and the fold itself), and the same for rows of which n doubles are wanted, written with a stride of
// bp_stats_row_stride(n)
size_t bp_stats_rows_bytes(int64_t rows, int C);
int bp_stats_rows_finish(double* ws, int64_t rows, int C, const IgemmStatsReq* sr, hipStream_t st);
int bp_stats_row_stride(int n);
size_t bp_stats_rows_bytes_n(int64_t rows, int n);
int bp_stats_rows_finish_n(double* ws, int64_t rows, int n, const IgemmStatsReq* sr, hipStream_t st);

// conv_ws_f32.hip: weights-stationary kernel of the 128 -> 128 k3 trunk layers (reads the tiled kernels' packed image)
void bp_f32_ws_set(int v);
bool bp_f32_ws_ok(const ConvGeom& g, const bp_view* in, const bp_view* out, const float* bias, int stats_mode);
size_t bp_f32_ws_stats_workspace(const ConvGeom& g, const bp_view* out);
int bp_f32_ws_run(const ConvGeom& g, const bp_view* in, const PW& pw, const float* packed_tiled, const bp_view* out,
                  hipStream_t st, const IgemmStatsReq* sr);

// conv_direct.hip
int bp_direct_gather(const ConvGeom& g, const WeightMap& wm, const bp_view* in, const PW& pw, const float* w_torch,
                     const float* bias, const bp_view* out, hipStream_t st);
int bp_direct_wgrad(const bp_conv* cv, const bp_view* X, const PW& pwx, const bp_view* Y, const PW& pwy, float* dst,
                    hipStream_t st);

// ---- weight gradient, fp32 and bf16: one record per kernel family (conv_wgrad.hip walks its two tables in priority
// order).  A call: X is the tensor on the fine grid, Y the one on the coarse grid (conv_wgrad.hip), each with the
// pointwise operand that lands on it; `shared`: the launch shares the GPU with another stream (BP_IMPL_SHARED).
struct WgradCall {
  const bp_conv* cv;
  const bp_view* X; PW pwx;
  const bp_view* Y; PW pwy;
  bool shared;
};
// What a family plans for a call it accepts: the BP_WG_* value of the kernel that runs (a family may hold several
// variants), its split count and workspace bytes.  Partial-sum kernels write ws[split][ky][kx][cyp][cxp]; the kernels that
// reduce themselves report their grid as nsplit and cxp = cyp = 0.
struct WgradRow {
  int id, nsplit, cxp, cyp;
  size_t bytes;
};
struct WgradFamily {
  const char* name;
  // is the call this family's layer, and if so its row: host arithmetic, no launch, pointers looked at for alignment only
  bool (*plan)(const WgradCall& c, WgradRow* row);
  // a call plan() accepted with `row`: partial sums into ws for conv_wgrad.hip to reduce in fixed order, or
  // (reduces_itself) dW into dst
  int (*run)(const WgradCall& c, const WgradRow& row, float* dst, void* ws, size_t ws_bytes, hipStream_t st);
  bool reduces_itself;
  // plan() may answer differently for the call than for its workspace query: the query passes no pointwise operand, and
  // bp_set_option may switch between the two.  The workspace is sized for the families after it as well, up to the
  // first acceptor without this flag.
  bool may_requalify;
};
// Most partial-sum kernels answer both questions with one function -- `dry`: fill *row, launch nothing;
// BP_EUNSUPPORTED: not this kernel's layer -- so that the plan and the launch are the same arithmetic.
using WgradPartialFn = int(const WgradCall& c, float* ws, size_t ws_bytes, WgradRow* row, hipStream_t st, bool dry);
template <WgradPartialFn* FN>
bool bp_wgrad_plan_of(const WgradCall& c, WgradRow* row) { return FN(c, nullptr, 0, row, nullptr, true) == BP_OK; }
template <WgradPartialFn* FN>
int bp_wgrad_run_of(const WgradCall& c, const WgradRow&, float*, void* ws, size_t ws_bytes, hipStream_t st) {
  WgradRow row;
  return FN(c, reinterpret_cast<float*>(ws), ws_bytes, &row, st, false);
}

// fp32.  conv_stem.hip: the 3 -> 16 k5 stem; conv_wgrad_flat.hip: the 16 -> 8 k7 head layer and the thin stride-2 k4
// layers (16 channels at full resolution, 32 at half) -- these three reduce their own partial sums
const WgradFamily& bp_wgrad_family_stem();
const WgradFamily& bp_wgrad_family_flat();
const WgradFamily& bp_wgrad_family_flat_s2();
// conv_wgrad_ws_f32.hip: output-stationary kernel of the 128 <-> 128 k3 trunk layers
const WgradFamily& bp_wgrad_family_ws_f32();
void bp_f32_wgrad_ws_set(int v);
// conv_enc.hip: the k8 stride-4 encoder layer
const WgradFamily& bp_wgrad_family_enc();
// conv_wgrad_thin.hip: one-channel tails (BP_WG_THIN_C1, BP_WG_THIN_CY1)
const WgradFamily& bp_wgrad_family_thin();
// conv_wgrad_small.hip: the tap-packed few-channel kernel, and the kernel itself for conv_wgrad.hip's chunked family
const WgradFamily& bp_wgrad_family_small();
WgradPartialFn bp_wgrad_small;
// conv_wgrad_tiles.hip: the tap-blocked kernels (BP_WG_TILES, BP_WG_TILES_DMA)
const WgradFamily& bp_wgrad_family_tiles();
// bf16.  conv_wgrad_bf16.hip: the heads' k7 layer, the generator's k5 stem, the heads' 8 -> 1 k5 tail, the tiled kernels
const WgradFamily& bp_wgrad_family_bf16_wf();
const WgradFamily& bp_wgrad_family_bf16_sf();
const WgradFamily& bp_wgrad_family_bf16_wh();
const WgradFamily& bp_wgrad_family_bf16_tiled();
// conv_wgrad_ws_bf16.hip: output-stationary kernel of the 128 <-> 128 k3 trunk layers
const WgradFamily& bp_wgrad_family_ws_bf16();
void bp_bf16_wgrad_ws_set(int v);

// conv_wgrad.hip: the two tables and their walk behind capi.hip, the fixed-order reduction and its deferral
struct WgradSelection {
  const WgradFamily* family;      // the first family that accepts the call, and its row
  WgradRow row;
  size_t ws_bytes;                // what a workspace query for this call answers (see WgradFamily::may_requalify)
};
int bp_wgrad_select(bool bf16, const WgradCall& c, WgradSelection* s);      // BP_OK / BP_EUNSUPPORTED
int bp_wgrad_run(const WgradSelection& s, const WgradCall& c, float* dst, void* workspace, size_t workspace_bytes,
                 hipStream_t st);
void bp_wgrad_private_ws(bool on);
int bp_wgrad_defer_begin_impl();
int bp_wgrad_defer_flush_impl(hipStream_t st, int end);

// conv_bf16.hip: the bf16 gather entry points behind capi.hip
bool bp_bf16_igemm_ok(const ConvGeom& g, const bp_view* in, const bp_view* out);
int64_t bp_bf16_packed_elems(const ConvGeom& g);
int bp_bf16_pack(const ConvGeom& g, const WeightMap& wm, const float* w_torch, void* packed, hipStream_t st);
int bp_bf16_igemm_run(const ConvGeom& g, const bp_view* in, const PW& pw, const void* packed, const float* bias,
                      const bp_view* out, hipStream_t st, const IgemmStatsReq* stats = nullptr);
size_t bp_bf16_stats_workspace(const ConvGeom& g, const bp_view* in, const bp_view* out, int mode);

// conv_bf16_flat.hip: flattened-K kernel for the unit-stride k7 head layers; its weight image follows the generic one
int64_t bp_bf16_flat_packed_elems(const ConvGeom& g);
int bp_bf16_flat_pack(const ConvGeom& g, const WeightMap& wm, const float* w_torch, uint16_t* dst, hipStream_t st);
bool bp_bf16_flat_ok(const ConvGeom& g, const bp_view* in, const bp_view* out, const float* bias, int stats);
size_t bp_bf16_flat_stats_workspace(const ConvGeom& g, const bp_view* in, const bp_view* out, int mode);
int bp_bf16_flat_run(const ConvGeom& g, const bp_view* in, const PW& pw, const uint16_t* packed_flat, const bp_view* out,
                     hipStream_t st, const IgemmStatsReq* sr);

// conv_bf16_ws.hip: weights-stationary kernel of the 128 -> 128 k3 trunk; its weight image follows the other two
void bp_bf16_ws_set(int v);
int bp_bf16_ws_kind(const ConvGeom& g);
int64_t bp_bf16_ws_packed_elems(const ConvGeom& g);
int bp_bf16_ws_pack(const ConvGeom& g, const WeightMap& wm, const float* w_torch, uint16_t* dst, hipStream_t st);
bool bp_bf16_ws_ok(const ConvGeom& g, const bp_view* in, const bp_view* out, const float* bias, int mode);
size_t bp_bf16_ws_stats_workspace(const ConvGeom& g, const bp_view* in, const bp_view* out);
int bp_bf16_ws_run(const ConvGeom& g, const bp_view* in, const PW& pw, const uint16_t* packed_ws, const bp_view* out,
                   hipStream_t st, const IgemmStatsReq* sr);

// conv_bf16_head.hip: data gradient (+ activation backward) of the heads' 8 -> 1 k5 layer; its weight image comes last
int64_t bp_bf16_head_packed_elems(const ConvGeom& g);
int bp_bf16_head_pack(const ConvGeom& g, const WeightMap& wm, const float* w_torch, uint16_t* dst, hipStream_t st);
bool bp_bf16_head_ok(const ConvGeom& g, const bp_view* in, const bp_view* out, const float* bias, int mode);
size_t bp_bf16_head_stats_workspace(const ConvGeom& g, const bp_view* in, const bp_view* out, int mode);
int bp_bf16_head_run(const ConvGeom& g, const bp_view* in, const uint16_t* packed_head, const bp_view* out,
                     hipStream_t st, const IgemmStatsReq* sr);

// pointwise.hip: sums of partial rows (the last stage of every statistics request)
int bp_sum_partials(const double* partial, int nblk, int n, double* out, hipStream_t st);
int bp_sum_partials_strided(const double* partial, int nblk, int stride, int n, double* out, hipStream_t st);
// ... partial[nblk][n] -> sr->sums (and, with sr->fin, the batch-norm finalize)
int bp_sum_partials_req(const double* partial, int nblk, int n, const IgemmStatsReq* sr, hipStream_t st);
int bp_sum_partials3(const double* partial, int nblk, int c, double* sums, hipStream_t st);

// assemble_gan.hip: the CGAN's training batch in one launch (an entry point of include/bp_hip.h defined in a file of its
// own; the descriptors and the pixel's value are assemble.hpp's, the transform is range_compress.hpp's rc_shift_log_cam)
int bp_gather_tiles_gan(const void* in100, const void* in150, const void* in_xform, const float* in_minima,
                        const void* lab100, const void* lab150, const void* lab_xform, const double* cam,
                        const float* aux, int32_t n, int32_t tile, const bp_view* gen_in, const bp_view* d_real,
                        const bp_view* d_fake_cond, float* x_nchw, void* stream);

// pointwise_bf16.hip: the streaming kernels on dense bf16 views
bool bp_bf16_dense_ok(const bp_view* v);
size_t bp_bf16_reduce_workspace(const bp_view* x, int nsums);
int bp_bf16_channel_sums(const bp_view* x, double* sums, void* workspace, hipStream_t st);
int bp_bf16_act_backward(const bp_view* dout, const bp_view* dout2, const bp_view* raw, const PW& pw,
                         const bp_view* act_out, const bp_view* g, double* sums, void* workspace, hipStream_t st);
int bp_bf16_bn_backward_apply(const bp_view* dout, const bp_view* dout2, const bp_view* raw, const PW& pw,
                              const bp_view* act_out, const double* abc, const bp_view* out, bool recompute_g,
                              hipStream_t st);
int bp_bf16_residual_forward(const bp_view* raw, const PW& pw, const bp_view* skip, const PW& spw, float slope,
                             const bp_view* out, hipStream_t st);
