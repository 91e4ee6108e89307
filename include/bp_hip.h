/*
 * bp_hip.h -- C ABI of the MI355X (gfx950) kernels behind the baryon_painter CVAE hot path.
 *
 * The reference has no FFI: its arithmetic boundary is the set of stock torch.nn modules that
 * `build_sequential` instantiates (/root/reference/baryon_painter/models/utils.py:114-157) plus
 * the tensor expressions in models/cvae.py:63-146.  Each entry point below replaces one of those
 * call sites (cited per function).  Signatures use plain pointers and sizes only; all buffers are
 * device memory owned by the caller, nothing is allocated or synchronised inside, every launch
 * goes to `stream` (a hipStream_t passed as void*), so a call sequence can be captured in a
 * hipGraph.  Return value: BP_OK or a negative error code; nothing is launched on error.
 *
 * Data layout: activations are NHWC fp32.  A `bp_view` addresses channels [coff, coff+c) of a
 * buffer whose pixels are `cstride` floats apart, so channel concatenation (cvae.py:72,109) is
 * "write into a slice".  Convolution outputs are stored RAW (pre batch-norm / pre activation);
 * the per-channel affine + leaky-ReLU that follows them in the module list (BatchNorm2d + ReLU /
 * PReLU / LeakyReLU) is described by a `bp_pointwise` and applied by the CONSUMER while it stages
 * its input ("lazy activation"), which keeps every activation at one HBM write + one read.
 */
#ifndef BP_HIP_H
#define BP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BP_OK 0
#define BP_EINVAL (-1)       /* inconsistent shapes / null pointers */
#define BP_EUNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define BP_ELAUNCH (-3)      /* hipGetLastError() != hipSuccess after the launch */
#define BP_EWORKSPACE (-4)   /* workspace too small */

/* Element type of a view.  fp32 is the reference's arithmetic (parity mode, BASELINE.json configs[1]); bf16
 * storage with fp32 accumulation is the throughput mode of configs[3] and is accepted by the entry points that say
 * so (convolutions, batch-norm statistics, activation / batch-norm backward, residual tail); every other entry
 * point returns BP_EUNSUPPORTED for a bf16 view. */
enum { BP_F32 = 0, BP_BF16 = 1 };

/* NHWC view: element (n,y,x,ch) lives at ptr[((n*h + y)*w + x)*cstride + coff + ch] (in elements of `dtype`). */
typedef struct bp_view {
  float* ptr;      /* device pointer (to 2-byte elements when dtype == BP_BF16) */
  int32_t n, h, w;
  int32_t c;       /* channels in this view            */
  int32_t cstride; /* channels of the underlying buffer */
  int32_t coff;    /* first channel of the view         */
  int32_t dtype;   /* BP_F32 (0) or BP_BF16             */
} bp_view;

/* Per-channel t = x*scale[ch] + shift[ch];  y = t > 0 ? t : t*slope[ch].
 * scale == NULL means identity (no transform at all).  ReLU: slope 0; PReLU: slope a;
 * identity-with-affine: slope 1.  Arrays have `c` entries of the view they accompany. */
typedef struct bp_pointwise {
  const float* scale;
  const float* shift;
  const float* slope;
} bp_pointwise;

/* torch.nn.Conv2d / ConvTranspose2d hyper-parameters (utils.py:128-131, square kernels). */
typedef struct bp_conv {
  int32_t transposed; /* 0: Conv2d, 1: ConvTranspose2d */
  int32_t cin, cout;  /* module in_channels / out_channels */
  int32_t k, stride, pad, out_pad;
} bp_conv;

enum { BP_IMPL_AUTO = 0, BP_IMPL_DIRECT = 1, BP_IMPL_MFMA = 2, BP_IMPL_BF16 = 3 };
/* OR-ed into `impl` of bp_conv_backward_weight: the launch shares the GPU with kernels of another stream (the
 * training step runs weight gradients beside the data-gradient chain), so persistent kernels take one workgroup
 * per CU instead of two and leave room for the other stream's workgroups (and the tiled weight gradients take fewer
 * split-K workgroups).  Results are deterministic per schedule; between the two schedules the grouping of tiles into
 * fp32 partial sums differs, so weight gradients may differ in their last bits. */
enum { BP_IMPL_SHARED = 0x100 };
/* OR-ed into `impl` of bp_conv_backward_weight between bp_wgrad_defer_begin / _flush: this call's workspace is not
 * touched by anyone else before the flush, so its split-K reduction may be deferred (see bp_wgrad_defer_begin). */
enum { BP_IMPL_DEFER = 0x200 };
enum { BP_PACK_FWD = 0, BP_PACK_BWD = 1 };

/* ---- library ------------------------------------------------------------------------------ */
int bp_version(void);
/* Kernel-selection switches for A/B measurements and tests inside ONE process (the environment variables of the same
 * names are read once, at the first call).  "bf16_ws" / "f32_ws": 1 / 0 = use / do not use the weights-stationary kernels
 * (csrc/conv_bf16_ws.hip: bf16 128 -> 128 k3 and 64 -> 128 k4 s2; csrc/conv_ws_f32.hip: fp32 128 -> 128 k3), -1 = back to the
 * environment's choice (BP_BF16_WS / BP_F32_WS); "f32_wgrad_ws" / "bf16_wgrad_ws": the output-stationary weight gradients of
 * the same trunk layers (csrc/conv_wgrad_ws_f32.hip, csrc/conv_wgrad_ws_bf16.hip; BP_F32_WGRAD_WS / BP_BF16_WGRAD_WS).
 * Not thread-safe against concurrent launches; results of either kernel meet the same tolerances.
 * Returns BP_EUNSUPPORTED for an unknown name. */
int bp_set_option(const char* name, int value);
const char* bp_strerror(int code);

/* ---- convolution (replaces nn.Conv2d / nn.ConvTranspose2d forward + their autograd backward,
 *      utils.py:128-131, painter.py:227) ----------------------------------------------------- */

/* Number of floats of the packed weight image for direction `dir` (BP_PACK_FWD feeds
 * bp_conv_forward, BP_PACK_BWD feeds bp_conv_backward_data). */
int64_t bp_conv_packed_floats(const bp_conv* cv, int dir);

/* Which igemm_kernel<CC,NT,WN,MT> instantiation serves this layer/direction, encoded as
 * CC*1000 + NT*100 + WN*10 + MT, plus 100000 / 200000 for the LDS-DMA pipelined igemm_dma_kernel with 4 / 8 waves and 300000 for
 * igemm_dmaf_kernel (tap groups, fused output phases)
 * (so a profile's kernel names can be matched to layers). */
int bp_conv_kernel_id(const bp_conv* cv, int dir);

/* Re-layout torch-format weights (Conv2d: [cout][cin][k][k]; ConvTranspose2d: [cin][cout][k][k])
 * into the MFMA image [phase][tap][cin_chunk][cout_pad][chunk] (zero padded).  Must be re-run
 * whenever the weights change (once per optimiser step). */
int bp_conv_pack(const bp_conv* cv, int dir, const float* w_torch, float* packed, void* stream);

/* Batched packing: every layer's weights in ONE launch (a step re-packs ~60 small images).  bp_conv_pack_job
 * fills a host record of bp_conv_pack_job_bytes() bytes describing bp_conv_pack(cv, dir, w_torch, packed) and
 * returns its workgroup count (BP_EUNSUPPORTED for the few layers served by the vector-ALU kernel: pack those
 * with bp_conv_pack).  The caller uploads the records back to back, plus first_block[njobs + 1] = exclusive
 * prefix sums of the workgroup counts, and launches them with bp_conv_pack_jobs; the pointers inside the records
 * must stay valid (parameters are views of one flat buffer, packed images belong to the plan). */
int32_t bp_conv_pack_job_bytes(void);
int bp_conv_pack_job(const bp_conv* cv, int dir, const float* w_torch, float* packed, void* job,
                     int64_t* nblocks);
int bp_conv_pack_jobs(const void* jobs_dev, const int64_t* first_block_dev, int32_t njobs,
                      int64_t total_blocks, void* stream);

/* bf16 matrix-core path (configs[3]): impl == BP_IMPL_BF16 in the three calls below takes a bf16 packed image
 * (bp_conv_bf16_pack, bp_conv_bf16_packed_elems 2-byte elements) and views of either element type on both sides;
 * products are bf16 x bf16, accumulation and the weight gradient are fp32.  bp_conv_bf16_supported says whether
 * the kernels take a layer / direction with the given views (NULL: any).  The packed image is opaque: for the thin
 * full-resolution layers (unit-stride k7 / k5 heads and stem, stride-2 k4 16<->32 and 32<->64) it carries a second,
 * flattened-K weight image behind the generic one (csrc/conv_bf16_flat.hip), and the run picks the kernel by the
 * views it is given -- always size the buffer with bp_conv_bf16_packed_elems.  bp_conv_bf16_supported answers for the tiled /
 * flattened-K kernels; the data gradient of the 8 -> 1 k5 head (fp32 dy, bf16 dx; csrc/conv_bf16_head.hip) reads its one
 * channel with scalar loads and also runs on dy views of any channel stride, for which the query says 0. */
int64_t bp_conv_bf16_packed_elems(const bp_conv* cv, int dir);
/* Which weights-stationary kernel serves this layer / direction with these views (`in` = the gathered tensor of the
 * direction: x for BP_PACK_FWD, dy for BP_PACK_BWD; `out` = the produced one): 3 = the k3 s1 128 -> 128 trunk kernel (bf16
 * views: csrc/conv_bf16_ws.hip; fp32 views: csrc/conv_ws_f32.hip), 4 = the bf16 strided gather k4 s2 64 -> 128, 5 = the bf16
 * transposed form k4 s2 128 -> 64, 0 = none
 * (the tiled / flattened-K kernels).  Widths: kind 3 takes 16, 32, 64 and, in 64-pixel column strips, wider multiples of 64 (bf16
 * views: 128, 192, 256; fp32 views: any; 128 is the CGAN generator's trunk at 512^2 tiles); kinds 4 and 5 take 16, 32, 64
 * on their coarse grid.  The answer never depends on the batch size.  For profiles and bench.py's kernel labels; follows bp_set_option. */
int bp_conv_ws_kind(const bp_conv* cv, int dir, const bp_view* in, const bp_view* out);
int bp_conv_bf16_pack(const bp_conv* cv, int dir, const float* w_torch, void* packed, void* stream);
int bp_conv_bf16_supported(const bp_conv* cv, int dir, const bp_view* in, const bp_view* out);

/* y_raw = conv(act(x)) [+ bias].  `x_pw` may be NULL (identity). */
int bp_conv_forward(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw,
                    const float* packed_fwd, const float* w_torch, const float* bias,
                    const bp_view* y, int impl, void* stream);

/* dx = d(loss)/d(act(x)) given dy = d(loss)/d(y_raw).  (The activation's own derivative is
 * applied afterwards by bp_act_backward.) */
int bp_conv_backward_data(const bp_conv* cv, const bp_view* dy, const float* packed_bwd,
                          const float* w_torch, const bp_view* dx, int impl, void* stream);

/* Convolution + per-channel sums in one launch (fp32 matrix-core kernels only): the sums are taken from the
 * accumulators in the kernel's epilogue, so the streaming pass of bp_channel_sums / bp_act_backward over the
 * produced tensor is not needed (batch-norm statistics of utils.py:146-147 and the two reductions of its backward).
 *   impl: BP_IMPL_MFMA (fp32 views) or BP_IMPL_BF16 (bf16 packed image, views of either type; forward only: the sums
 *       are those of the tensor as stored, i.e. of the bf16-rounded values where y is bf16).
 *   bp_conv_stats_workspace(cv, dir, x, y, impl)  bytes of workspace for layer `cv` on module input x / output y
 *       (BP_PACK_FWD: bp_conv_forward_stats, BP_PACK_BWD: bp_conv_backward_data_stats); 0 = this layer's kernel
 *       has no statistics epilogue (bias, pixel-packed or vector-ALU kernels, channel count not a power of two):
 *       use the separate passes.
 *   bp_conv_forward_stats        y_raw = conv(act(x)); sums[2*cout] = {sum y, sum y^2} as bp_channel_sums(y).
 *   bp_conv_backward_data_stats  dx = d(loss)/d(act(x)) as bp_conv_backward_data; sums[2*cin] = {sum g, sum g*x_raw},
 *       g = dx * act'(x_pw(x_raw)): the first two sums of bp_act_backward(dx, NULL, x_raw, x_pw, ...).  With bf16
 *       views (dx and x_raw bf16, packed_bwd the bf16 image) the bf16 kernels run: their two full-resolution
 *       flattened-K data gradients have the epilogue (the layers behind the generator's 16-channel 512^2 slots), g
 *       from the bf16-rounded dx as stored; workspace query with impl = BP_IMPL_BF16. */
size_t bp_conv_stats_workspace(const bp_conv* cv, int dir, const bp_view* x, const bp_view* y, int impl);
int bp_conv_forward_stats(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw, const float* packed_fwd,
                          const bp_view* y, double* sums, void* workspace, size_t workspace_bytes, int impl,
                          void* stream);
int bp_conv_backward_data_stats(const bp_conv* cv, const bp_view* dy, const float* packed_bwd, const bp_view* dx,
                                const bp_view* x_raw, const bp_pointwise* x_pw, double* sums, void* workspace,
                                size_t workspace_bytes, void* stream);

/* Data gradient + the producer's WHOLE activation backward in one launch, for a producer without batch-norm (the
 * heads' PReLU layers, cvae.py:57-58 via utils.py:135): what is stored is g = dx * act'(x_pw(x_raw)) -- exactly what
 * bp_act_backward(dx, NULL, x_raw, x_pw, NULL, g = dx, ...) would leave in place of dx -- and sums[3*cin] are its
 * three sums {sum g, sum g*x_raw, sum_{t<=0} dx*t} (the last is the PReLU slope gradient, bp_prelu_slope_grad).
 * Saves the separate pass' read of dx and its write of g (x_raw is read either way).
 * bp_conv_backward_data_act_workspace: bytes of workspace, 0 = this layer's kernel has no such epilogue (only the
 * vector-ALU kernel of the 8 -> 1 k5 layer has one: 0.35 ms of a 15 ms bf16 step). */
size_t bp_conv_backward_data_act_workspace(const bp_conv* cv, const bp_view* dy, const bp_view* g);
int bp_conv_backward_data_act(const bp_conv* cv, const bp_view* dy, const float* packed_bwd, const bp_view* g,
                              const bp_view* x_raw, const bp_pointwise* x_pw, double* sums, void* workspace,
                              size_t workspace_bytes, void* stream);

/* bp_conv_forward_stats followed by bp_bn_finalize(sums, ...) of the produced tensor, with the finalize folded into
 * the launch that sums the epilogue's partial rows (one small launch less per batch-norm layer and step; the same
 * numbers bit for bit).  Single-device training only: under data parallelism the sums are all-reduced between the two
 * calls (utils.py:146-147 on the global batch).  The fields are bp_bn_finalize's arguments. */
typedef struct bp_bn_train {
  double count;                       /* elements per channel: n * h * w of y */
  const float* gamma; const float* beta; /* NULL: 1 / 0 */
  float eps, momentum;
  float* running_mean; float* running_var; int64_t* num_batches_tracked; /* updated in place; NULL: skipped */
  float* scale; float* shift;         /* the pending batch-norm of y as a bp_pointwise */
  double* save_mean; double* save_invstd; /* for bp_bn_backward_finalize; NULL: skipped */
} bp_bn_train;
int bp_conv_forward_bn(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw, const float* packed_fwd,
                       const bp_view* y, double* sums, const bp_bn_train* bn, void* workspace, size_t workspace_bytes,
                       int impl, void* stream);

/* dw (torch layout, overwritten) and optionally dbias (NULL to skip) from act(x) and dy. */
size_t bp_conv_backward_weight_workspace(const bp_conv* cv, const bp_view* x, const bp_view* dy);
int bp_conv_backward_weight(const bp_conv* cv, const bp_view* x, const bp_pointwise* x_pw,
                            const bp_view* dy, float* dw_torch, float* dbias, void* workspace,
                            size_t workspace_bytes, int impl, void* stream);

/* Which kernel bp_conv_backward_weight would run for these views and this `impl` (BP_IMPL_SHARED included; options set
 * with bp_set_option are honoured), and with how many partial images: out = {family, nsplit, cxp, cyp}.  Host arithmetic
 * only: nothing is launched and no view pointer is dereferenced (its alignment is looked at).  `family` is one of the
 * values below, one per file-level kernel; `nsplit` is the number of partial images the kernel writes (for the kernels
 * that reduce themselves -- stem, flat, flat_s2 -- their grid; 0 for the direct kernel); cxp x cyp are the padded
 * channel counts of one partial image (0 where the kernel has no such image; for the chunked kernel: of one chunk).
 * A pending activation does not enter the choice.  Returns what the call would return before its first launch
 * (BP_EUNSUPPORTED: no kernel; then out is {-1, 0, 0, 0}). */
enum {
  BP_WG_WS_F32 = 0, BP_WG_ENC, BP_WG_THIN_C1, BP_WG_THIN_CY1, BP_WG_SMALL, BP_WG_SMALL_CHUNKED, BP_WG_TILES,
  BP_WG_TILES_DMA, BP_WG_GENERAL, BP_WG_STEM, BP_WG_FLAT, BP_WG_FLAT_S2, BP_WG_DIRECT, BP_WG_BF16_TILED, BP_WG_BF16_WF,
  BP_WG_BF16_SF, BP_WG_BF16_WH, BP_WG_WS_BF16
};
int bp_conv_backward_weight_plan(const bp_conv* cv, const bp_view* x, const bp_view* dy, int impl, int32_t out[4]);

/* Deferred split-K reductions.  Between bp_wgrad_defer_begin() and bp_wgrad_defer_flush(end = 1, ...) on one host
 * thread, a bp_conv_backward_weight call flagged BP_IMPL_DEFER launches the layer's partial-sum kernel but only
 * RECORDS its reduction into dw_torch;
 * bp_wgrad_defer_flush launches every recorded reduction on `stream` (two launches for a whole network instead of
 * one per layer; each dw is reduced in the same order as without deferral: bit-identical).  The caller must give each
 * flagged call its own workspace until the flush, and flush on the stream (or behind the streams) the calls ran on.
 * Measured on the fiducial step: -0.3 ms for the fp32 layers (28-way splits, partial sums of 0.6 ... 16 MB); the
 * 128 ... 512-way splits of the bf16 kernels are better reduced at once, while their partial sums are still in L2.
 * end = 0 flushes and keeps deferring; end < 0 drops what was recorded and stops (error paths).  The recorded state is
 * per host thread: a flush (end >= 0) on a thread without an active bp_wgrad_defer_begin returns BP_EINVAL instead of
 * silently leaving the deferred gradients unreduced.  (Replaces nothing in the reference: torch's autograd launches one cuDNN
 * weight-gradient kernel per layer, cvae.py:392 loss.backward().) */
int bp_wgrad_defer_begin(void);
int bp_wgrad_defer_flush(int end, void* stream);

/* ---- batch norm (replaces nn.BatchNorm2d, utils.py:146-147) -------------------------------- */

/* Per-channel double sums[2*c] = {sum x, sum x^2} over all pixels of `x` (deterministic two-stage
 * reduction).  workspace: bp_channel_sums_workspace(x) bytes.  Under data parallelism the caller
 * all-reduces `sums` across ranks before bp_bn_finalize (global-batch statistics). */
size_t bp_channel_sums_workspace(const bp_view* x);
int bp_channel_sums(const bp_view* x, double* sums, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Train mode: batch mean / biased variance from `sums` and `count` (= N*H*W over all ranks),
 * writes the consumer's pointwise (scale = gamma*invstd, shift = beta - mean*scale), saves
 * mean/invstd (in double: the backward's cancellation needs them exact) for backward and updates running stats (momentum, unbiased variance) and
 * num_batches_tracked (int64, may be NULL). */
int bp_bn_finalize(const double* sums, double count, int32_t c, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean,
                   float* running_var, int64_t* num_batches_tracked, float* scale, float* shift,
                   double* save_mean, double* save_invstd, void* stream);

/* Eval mode: scale/shift from the running statistics. */
int bp_bn_eval_pointwise(int32_t c, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps,
                         float* scale, float* shift, void* stream);

/* ---- activation / batch-norm backward ------------------------------------------------------ */

/* Backward through y = leaky(raw*scale+shift [+ skip], slope):
 *   g = (dout [+ dout2]) * act'(t)           written to `g` (may alias dout; NULL: sums only, for
 *                                            layers that continue with bp_act_bn_backward_apply)
 *   sums[3*c] (double) = { sum g, sum g*raw, sum (dout[+dout2]) * t * [t<=0] }  (third: d slope)
 * `act_out`, if given, is the saved activated output and supplies the sign of t (residual
 * blocks, where t includes the skip); otherwise t is recomputed from raw and `pw`. */
size_t bp_act_backward_workspace(const bp_view* raw);
int bp_act_backward(const bp_view* dout, const bp_view* dout2, const bp_view* raw,
                    const bp_pointwise* pw, const bp_view* act_out, const bp_view* g,
                    double* sums, void* workspace, size_t workspace_bytes, void* stream);

/* bp_act_backward followed by bp_bn_backward_finalize(sums, ...) of the same layer, the finalize folded into the
 * launch that adds the partial sums (one tiny launch less per batch-norm layer on the backward chain, where every
 * launch's latency is exposed; the same numbers bit for bit).  Single-device training only: under data parallelism
 * the sums are all-reduced between the two.  The fields are bp_bn_backward_finalize's arguments. */
typedef struct bp_bn_backward_fin {
  double count;
  const float* gamma;                    /* NULL: 1 */
  const double* save_mean; const double* save_invstd;
  float param_grad_scale;
  float* dgamma; float* dbeta;           /* NULL: skipped */
  double* coef_abc;                      /* [4*c] */
} bp_bn_backward_fin;
int bp_act_backward_bn(const bp_view* dout, const bp_view* dout2, const bp_view* raw,
                       const bp_pointwise* pw, const bp_view* act_out, const bp_view* g, double* sums,
                       const bp_bn_backward_fin* fin, void* workspace, size_t workspace_bytes, void* stream);

/* From the (all-reduced) sums: dgamma, dbeta and the per-channel coefficients {A, mg, B, mean} of
 *   d_raw = A*(g - mg) + B*(raw - mean)   (batch-norm backward as an affine map of (g, raw)),
 * kept and evaluated in double like the reference's CPU batch_norm_backward (its accumulate type).
 * dgamma/dbeta are multiplied by `param_grad_scale` (1/world_size under data parallelism, where
 * the sums are global but every rank's loss is normalised by its local batch; 1 otherwise). */
int bp_bn_backward_finalize(const double* sums, double count, int32_t c, const float* gamma,
                            const double* save_mean, const double* save_invstd,
                            float param_grad_scale, float* dgamma, float* dbeta,
                            double* coef_abc /* [4*c] */, void* stream);

/* out = A*(g - mg) + B*(raw - mean)  (out may alias g). */
int bp_bn_backward_apply(const bp_view* g, const bp_view* raw, const double* coef_abc,
                         const bp_view* out, void* stream);

/* The same map with g recomputed on the fly from (dout [+ dout2], raw, pw, act_out) exactly as
 * bp_act_backward defines it: pairs with bp_act_backward(..., g = NULL, ...) so that g never
 * travels through HBM (out may alias dout). */
int bp_act_bn_backward_apply(const bp_view* dout, const bp_view* dout2, const bp_view* raw,
                             const bp_pointwise* pw, const bp_view* act_out, const double* coef_abc,
                             const bp_view* out, void* stream);

/* dst[ch] = (float) sums[ch]  (e.g. a bias gradient from bp_channel_sums of dy). */
int bp_sums_to_float(const double* sums, int32_t c, float* dst, void* stream);

/* PReLU slope gradient (one shared slope, utils.py:137): dslope = sum over channels of sums[2]. */
int bp_prelu_slope_grad(const double* sums, int32_t c, float* dslope, void* stream);

/* ---- residual block tail (utils.py:35-37): out = leaky(raw*scale+shift + act(skip), slope) -- */
int bp_residual_forward(const bp_view* raw, const bp_pointwise* pw, const bp_view* skip,
                        const bp_pointwise* skip_pw, float slope, const bp_view* out, void* stream);

/* ---- element type conversion: dst = act(src*scale+shift) (pw NULL: dst = src), fp32 -> bf16 (round to nearest even,
 * after the pointwise, which is evaluated in fp32) or bf16 -> fp32 (exact).  Views of any channel stride / offset; 16
 * bytes per lane where both have channel counts, strides and offsets that are multiples of 8 and 16-byte aligned bases.
 * BP_EINVAL for views of one element type or of different shapes. */
int bp_view_cast(const bp_view* src, const bp_pointwise* pw, const bp_view* dst, void* stream);

/* ---- layout glue ---------------------------------------------------------------------------- */

/* NCHW (N,c,H,W) -> channels [coff, coff+c) of `out`, and the aux label(s) (N,caux) broadcast to
 * constant planes in the next caux channels (merge_aux_label, utils.py:159-182). aux may be NULL. */
int bp_nchw_to_view(const float* src_nchw, int32_t c, const float* aux, int32_t caux,
                    const bp_view* out, void* stream);
/* dst = [softplus](act(src)) as NCHW; `softplus` = 1 applies torch's Softplus(beta=1,threshold=20). */
int bp_view_to_nchw(const bp_view* src, const bp_pointwise* pw, int32_t softplus, float* dst_nchw,
                    void* stream);
int bp_fill(float* dst, int64_t n, float value, void* stream);
/* h_y.repeat(L, 1, 1, 1) of cvae.py:109 and its adjoint, on channel-slice views (fp32; dst->n == L * src->n, same h, w, c):
 *   bp_repeat_samples        : dst[l * n + m] = src[m] for l < L.  RAW values: a batch-norm / activation pending on
 *                              the slice applies to every copy alike
 *   bp_repeat_samples_adjoint: d_src[m] = ((d_dst[m] + d_dst[n + m]) + d_dst[2 n + m]) + ... in float32, ascending l:
 *                              the same inputs give the same bits
 * 16-byte accesses where c, both channel strides and both offsets are multiples of 4 and both bases 16-byte aligned,
 * one float per access otherwise.  BP_EINVAL before anything is written for a malformed or bf16 view or L < 1. */
int bp_repeat_samples(const bp_view* src, int32_t L, const bp_view* dst, void* stream);
int bp_repeat_samples_adjoint(const bp_view* d_dst, int32_t L, const bp_view* d_src, void* stream);

/* ---- paint() pipeline (painter.py:371-392 around cvae.py:149-162; utils/data_transforms.py:72-97) ----------------
 * The raw tile goes in, the physical tile comes out: the reference's "shift-log" range compression and its inverse
 * are fused into the layout kernels on either side of the network, with the float32 / float64 promotion of the
 * reference's NumPy expressions, so device and host transforms agree bit for bit up to libm's exp (<= 1 ulp).
 *   bp_paint_load : out[n,:,:,ch<c] = (float) (log((double) raw / sigma_k[n][0] + 1) / sigma_k[n][1]), and the aux
 *                   label(s) as constant planes in the next caux channels (= transform + bp_nchw_to_view)
 *   bp_paint_store: dst = (float) ((double) (expf32(act(src) * (float) k_sigma[n][0]) - 1.f) * k_sigma[n][1]),
 *                   NCHW (= bp_view_to_nchw + inverse transform; softplus as in bp_view_to_nchw) */
int bp_paint_load(const float* raw_nchw, int32_t c, const double* sigma_k, const float* aux, int32_t caux,
                  const bp_view* out, void* stream);
/* bp_paint_load into TWO views of the same shape at once (cvae.py:87-88 and :104-105 merge the same y with the aux
 * label for the prior network and for the generator's concatenated input): one evaluation of the transform. */
int bp_paint_load2(const float* raw_nchw, int32_t c, const double* sigma_k, const float* aux, int32_t caux,
                   const bp_view* out, const bp_view* out2, void* stream);
int bp_paint_store(const bp_view* src, const bp_pointwise* pw, int32_t softplus, const double* k_sigma,
                   float* dst_nchw, void* stream);
/* ---- the six range-compression modes (utils/data_transforms.py: _MODES; csrc/range_compress.hpp) -----------------
 * The `_mode` forms of the transform-carrying entry points take one mode per launch (a painter has one per field) and
 * `records`: device, (n, 4) float64 {s, k, c, b} per tile, every constant computed on the host in float64
 * (data_transforms.DeviceRangeCompress.records), so host and device share the branch values exactly:
 *   BP_RC_SHIFT_LOG    {std, k, -, -}             log(x/std + 1)/k
 *   BP_RC_LOG          {std, k, eps, log(eps)/k}  x > 0 ? log(x/std + eps)/k : log(eps)/k
 *   BP_RC_SHIFT_LOG_2P {std, k[1], k[0], -}       log(x/std + k[0])/k[1]
 *   BP_RC_LOG_TANH     {std, k, eps, -}           x > 0 ? tanh(log(x/std + eps)/k) : -1
 *   BP_RC_X_1PX        {std, k[0], k[1], -}       x/(x + std)*k[0] - k[1]
 *   BP_RC_INV_X        {std*mean*k, k, mean, std} t = x/(std*mean*k); t > -1 ? 2/(t + 1) - 1.001 : -1
 * Forward is evaluated in float64 and rounded to float32 once; the inverses follow the host's float32 / float64
 * promotion for a float32 activation (DESIGN.md has the table); a NaN takes the branch np.where takes.  The entry points
 * without `_mode` are these at BP_RC_SHIFT_LOG over their tables of two doubles: same kernels, same bits as before.
 * An unknown mode is BP_EINVAL and a bf16 view BP_EUNSUPPORTED, both before anything is written; otherwise arguments,
 * limits and error order are those of the form without `_mode`. */
enum { BP_RC_SHIFT_LOG = 0, BP_RC_LOG = 1, BP_RC_SHIFT_LOG_2P = 2, BP_RC_LOG_TANH = 3, BP_RC_X_1PX = 4, BP_RC_INV_X = 5 };
int bp_paint_load_mode(int32_t mode, const float* raw_nchw, int32_t c, const double* records, const float* aux,
                       int32_t caux, const bp_view* out, void* stream);
int bp_paint_load2_mode(int32_t mode, const float* raw_nchw, int32_t c, const double* records, const float* aux,
                        int32_t caux, const bp_view* out, const bp_view* out2, void* stream);
int bp_paint_store_mode(int32_t mode, const bp_view* src, const bp_pointwise* pw, int32_t softplus,
                        const double* records, float* dst_nchw, void* stream);
/* The same pair for the conditional GAN (painter.CGANPainter: the "shift-log-cam" transform into the tanh range and
 * the generator's tanh head), everything after the float32 tanh in double, as the host's NumPy expressions:
 *   bp_paint_load_cam : out[n,:,:,ch<c] = (float) (log((double) raw / xf[n][0] + 1) / xf[n][1] - xf[n][2]), xf (n,3)
 *                       double {sigma, k0, k1}; the aux label(s) (n,caux), read from device memory (the caller stores
 *                       z - 1 there), as constant planes in the next caux channels, as in bp_paint_load
 *   bp_paint_store_cam: dst = (float) ((exp(((double) tanhf(src) + xf[n][1]) * xf[n][0]) - 1) * xf[n][2]), NCHW, xf
 *                       (n,3) double {k0, k1, sigma}; tanhf is bp_unary_forward's (kind 1)
 * fp32 views only: BP_EUNSUPPORTED for a bf16 view; BP_EINVAL (nothing written) as in bp_paint_load / bp_paint_store. */
int bp_paint_load_cam(const float* raw_nchw, int32_t c, const double* xf, const float* aux, int32_t caux,
                      const bp_view* out, void* stream);
int bp_paint_store_cam(const bp_view* src, const double* xf, float* dst_nchw, void* stream);
/* ---- split-scale (Gaussian pyramid) transform (utils/data_transforms.py: create_split_scale_transform) ----------
 * The pyramid of a float32 tile x: d = x; for i = n_scale-1 .. 1: g = gaussian_filter(d, sigma_i); scale i = g;
 * d -= g; scale 0 = d.  Channel order: [x if include_original] scale 0 .. scale n_scale-1, `levels` = n_scale +
 * include_original channels.  The filter is scipy.ndimage.gaussian_filter's on float32 input: weights
 * exp(-0.5 k^2 / sigma^2), k = -r .. r, divided by their float64 sum, r = int(truncate * sigma + 0.5); axis 0 first,
 * then axis 1; each axis accumulates in float64 and is rounded to float32 once; boundary "reflect" (d c b a | a b c d),
 * folded with period 2n when r exceeds the line; d -= g is a float32 subtraction.
 *   weights : device, float64: the 2 r_i + 1 weights of level 1, then those of level 2, ... (computed on the host
 *             with SciPy's expression: data_transforms.gaussian_weights); radii: HOST array of n_scale int32, entry
 *             i = r_i (entry 0 is not read).  Both may be NULL for n_scale = 1.
 *   scratch : bp_split_scale_workspace(n, h, w) bytes (three float32 planes of the batch), BP_EWORKSPACE if shorter
 *   bp_split_scale       : tiles (n, h, w) float32 (rectangular tiles allowed) -> channels [coff, coff + levels) of
 *                          `out` (out->c == levels, out->n/h/w == n/h/w); other channels of the buffer are not touched
 *   bp_paint_load_scales2: bp_paint_load2 with the pyramid between the transform and the layout: raw (n, 1, H, W) ->
 *                          the float32 shift-log value of bp_paint_load -> its pyramid in the first `levels` channels
 *                          of BOTH views, the aux planes in the next caux (out->c == levels + caux)
 *   bp_paint_store_scales: bp_paint_store for a `levels`-channel head (src->c == levels): activation and softplus per
 *                          channel, then channel 0 (include_original) or the float32 sum ((c0 + c1) + c2) ... in
 *                          channel order (NumPy's sum(axis=0)), then bp_paint_store's inverse shift-log expression
 *                          unchanged; dst (n, 1, H, W)
 * fp32 views only (BP_EUNSUPPORTED for a bf16 view, for radii whose halo does not fit the 64 KiB of LDS a launch may
 * ask for -- r <= 96 -- and for more than 16 scales); BP_EINVAL / BP_EUNSUPPORTED / BP_EWORKSPACE are returned before
 * anything is written.  No atomics (the same inputs give the same bits), no host synchronisation. */
size_t bp_split_scale_workspace(int32_t n, int32_t h, int32_t w);
int bp_split_scale(const float* tiles, int32_t n, int32_t h, int32_t w, int32_t n_scale, int32_t include_original,
                   const double* weights, const int32_t* radii, void* scratch, size_t scratch_bytes,
                   const bp_view* out, void* stream);
int bp_paint_load_scales2(const float* raw_nchw, const double* sigma_k, const float* aux, int32_t caux,
                          int32_t n_scale, int32_t include_original, const double* weights, const int32_t* radii,
                          void* scratch, size_t scratch_bytes, const bp_view* out, const bp_view* out2, void* stream);
int bp_paint_store_scales(const bp_view* src, const bp_pointwise* pw, int32_t softplus, int32_t include_original,
                          const double* k_sigma, float* dst_nchw, void* stream);
/* bp_paint_load_scales2 / bp_paint_store_scales with any range-compression mode (see bp_paint_load_mode). */
int bp_paint_load_scales2_mode(int32_t mode, const float* raw_nchw, const double* records, const float* aux,
                               int32_t caux, int32_t n_scale, int32_t include_original, const double* weights,
                               const int32_t* radii, void* scratch, size_t scratch_bytes, const bp_view* out,
                               const bp_view* out2, void* stream);
int bp_paint_store_scales_mode(int32_t mode, const bp_view* src, const bp_pointwise* pw, int32_t softplus,
                               int32_t include_original, const double* records, float* dst_nchw, void* stream);
/* The store of a head that paints several label fields at once (painter.CVAEPainter with len(label_fields) > 1): field
 * f owns channels [f * levels, (f + 1) * levels) of `src` (src->c == fields * levels) and plane f of dst
 * (n, fields, H, W).  Per field the arithmetic is bp_paint_store_mode's for levels == 1 and
 * bp_paint_store_scales_mode's for levels > 1 -- activation and softplus per channel, channel 0 (include_original) or
 * the float32 sum ((c0 + c1) + c2) ..., then the inverse of mode modes[f] with the field's record -- and the bits are
 * those of these entry points on the field's channel-slice view (pw, where given, holds fields * levels channels).
 *   modes   : HOST array of `fields` int32 (BP_RC_*), held as a constant of the launch
 *   records : device, (n, fields, 4) float64: DeviceRangeCompress.records of each field
 * include_original has no effect at levels == 1.  One launch; a head value is read by one thread.  Before anything is
 * written: BP_EINVAL for a null pointer or a malformed view, fields < 1, levels < 1, src->c != fields * levels or a mode
 * outside 0 ... 5; then BP_EUNSUPPORTED for a bf16 view, more than 16 levels, more than 64 fields or
 * n * H * W * src->c >= 2^31.  No atomics, no host synchronisation. */
int bp_paint_store_fields(const int32_t* modes, int32_t fields, int32_t levels, int32_t include_original,
                          const bp_view* src, const bp_pointwise* pw, int32_t softplus, const double* records,
                          float* dst_nchw, void* stream);
/* The store of an ENSEMBLE (painter.CVAEPainter.paint_ensemble): `src` is a head of draws * n samples, sample l * n + m
 * = draw l of tile m (the order of a plan with `draws` latent samples per input), src->c == fields * levels.  With p_l
 * the float32 value bp_paint_store_fields writes for sample l * n + m under tile m's record -- the same device
 * functions, the same bits -- per tile m, field f and pixel, in float64 without contraction, ascending l:
 *   S = ((p_0 + p_1) + ...) + p_{K-1},  M = S / K,  Q = ((p_0 - M)^2 + (p_1 - M)^2) + ...,  K = draws
 *   mean_nchw = (float) M,  var_nchw = (float) (Q / K)      (n, fields, H, W) each: the population variance, np.var's
 * Non-finite values get no special handling (an infinite draw: mean +-inf, var NaN, as NumPy); draws == 1 gives
 * var == +0 for a finite p_0.
 *   modes      : HOST array of `fields` int32 (BP_RC_*), as in bp_paint_store_fields
 *   records    : device, (n, fields, 4) float64, one row per TILE
 *   draws_nchw : NULL, or (n, draws, fields, H, W), tile-major: receives every p_l
 * One launch, one thread per tile pixel (four pixels and 16-byte accesses for a one-channel head with cstride 1, planes
 * of a multiple of four pixels and 16-byte aligned pointers); up to 16 draws stay in registers between the two sums,
 * more are read and evaluated a second time.  No atomics, no workspace, no host synchronisation: the same inputs give
 * the same bits.  Before anything is written: BP_EINVAL for a null pointer other than pw or draws_nchw, a malformed
 * view, fields < 1, levels < 1, draws < 1, src->c != fields * levels, src->n % draws != 0 or a mode outside 0 ... 5;
 * then BP_EUNSUPPORTED for a bf16 view, draws > 64, levels > 16, fields > 64 or src->n * H * W * src->c >= 2^31. */
int bp_paint_store_moments(const int32_t* modes, int32_t fields, int32_t levels, int32_t include_original,
                           const bp_view* src, const bp_pointwise* pw, int32_t softplus, const double* records,
                           int32_t draws, float* mean_nchw, float* var_nchw, float* draws_nchw, void* stream);
/* eps (L, n, per_tile) standard normal for the sampler of cvae.py:64-65 from Philox4x32-10 keyed on `seed`, counter
 * (element group, l, tile id): a tile's noise depends on (seed, its GLOBAL id) only, not on batch, stream or rank
 * (torch.randn on the device in the reference: same distribution, no reproducible stream to match). */
int bp_philox_normal(uint64_t seed, const int64_t* tile_ids, int32_t n, int32_t L, int32_t per_tile, float* eps,
                     void* stream);
/* The same with the key read from device memory at run time: a launch captured in a hipGraph then serves every seed
 * (the reference draws fresh torch.randn per tile, cvae.py:64: planes of a light cone must not share their noise). */
int bp_philox_normal_dev(const uint64_t* seed_dev, const int64_t* tile_ids, int32_t n, int32_t L, int32_t per_tile,
                         float* eps, void* stream);
/* A draw from the likelihood of a CVAE with a variance head (painting with pixel noise): for every element
 * (n, y, x, ch) of three fp32 views of equal (n, h, w, c), any cstride and coff,
 *   t = softplus ? softplus(mu) : mu          (bp_paint_store's expression)
 *   out = t + expf(0.5f * log_var) * e        (float32; the product and the sum each round once; where the product is
 *                                              zero, out is t itself, the sign of a zero and a NaN's payload included)
 * e is the float32 value of the r-th Box-Muller normal (in double, as bp_philox_normal's) of the Philox4x32-10 block
 * with key *seed_dev and counter (X + ((ch / 4) << 24), 0x80000000 | Y, id low, id high), r = ch % 4,
 * Y = origins[n][0] + y, X = origins[n][1] + x, id = noise_ids[n].  The counter is a pixel of a noise LATTICE: samples
 * with one id whose origins put them over the same lattice pixel get the same e there (the overlapping tiles of a plane).
 * Bit 31 of counter word 1 keeps these blocks apart from bp_philox_normal's (l < 2^31) under the same key.
 *   seed_dev  : device, read at run time (a captured launch serves every seed)
 *   noise_ids : device, (n) int64
 *   origins   : device, (n, 2) int32 {row, col}, or NULL for all zero
 * `out` may be `mu` or `log_var` itself (each element is read and written by one thread).  Before anything is
 * launched: BP_EINVAL for a null pointer other than `origins`, a malformed view or views that differ in n, h, w or c;
 * then BP_EUNSUPPORTED for a bf16 view or n * h * w * c >= 2^31.  THE CALLER GUARANTEES what cannot be checked without
 * reading device memory: origins >= 0, X < 2^24 and Y < 2^31 for every element (beyond them lattice pixels share
 * their counters).  One launch, no atomics, no workspace, no host synchronisation. */
int bp_likelihood_draw(const bp_view* mu, int32_t softplus, const bp_view* log_var, const uint64_t* seed_dev,
                       const int64_t* noise_ids, const int32_t* origins, const bp_view* out, void* stream);

/* ---- light-cone planes (lightcone.paint_plane(on_device=True), process_SLICS.py:198-220) -----------------------
 * A periodic plane is cut into the paint graph's raw tiles, and the painted tiles are blended into float64 planes, on
 * the device: the plane goes up once and only the finished plane comes back.  Integers (cut origins, destinations,
 * bounding boxes) are computed on the host with lightcone.get_tile / generate_tiling's expressions.
 *   bp_plane_cut   : out[t] (n, tile, tile) float32 = the cut x cut block of `plane` (rows x cols, BP_F32 or BP_F64)
 *                    at origins[t] = {x0, y0} (device, int32 (n, 2)), rows wrapped modulo `rows`, columns modulo
 *                    `cols`.  cut == tile: a gather, bit-exact to get_tile + astype(float32).  cut != tile:
 *                    scipy.ndimage.zoom(cut_block, tile / cut, order=3, mode="reflect") in float64 (spline prefilter
 *                    along axis 0 then axis 1, tensor-product sampling at k (cut - 1) / (tile - 1)), rounded once to
 *                    float32; needs bp_plane_cut_workspace(n, cut, tile) bytes of `scratch` (less works in chunks of
 *                    tiles, down to one tile's share; BP_EWORKSPACE below that).  What is computed is the exact cubic
 *                    spline under half-sample symmetric boundaries (the prefilter solves
 *                    (c[k-1] + 4 c[k] + c[k+1]) / 6 = s[k] to rounding).  For cut >= 12 that is SciPy's zoom to
 *                    1 float32 ulp.  Below 12 SciPy's own "reflect" prefilter departs from the exact solve, and the
 *                    device differs from the host path (SciPy) by that much, relative to the tile's largest value
 *                    (measured on the CPU, SciPy 1.15.3, tests/test_plane_kernels_host.py):
 *                      cut   2     3     4     5     6     7     8     9     10    12    14
 *                            6e-4  1e-4  7e-6  3e-7  5e-8  2e-9  3e-10 1e-11 5e-13 7e-15 2e-15
 *                    BP_EINVAL for a null plane, origins or out, rows, cols, n, cut or tile <= 0, a dtype other than
 *                    BP_F32 / BP_F64 and, where cut != tile, a null scratch or cut or tile of 1; then
 *                    BP_EUNSUPPORTED for rows * cols, n * tile^2 or n * cut^2 >= 2^31; then BP_EWORKSPACE.  Nothing
 *                    is written on a refusal
 *   bp_plane_blend : for t = 0 .. n-1 in order, acc[dst[t] + (i, j)] += w[i, j] * (double) tiles[t][i, j] and
 *                    wsum[...] += w[i, j], over the plane pixels of the bounding box [bx0, bx1) x [by0, by1) (pixels
 *                    of a tile outside it are not blended).  `weight` is the float64 (tile, tile) feathering map.
 *                    regularise != 0: w = 0 where |p - mean| > std * regularise_std, with the tile's mean and
 *                    population std in float64 (fixed-order reduction into stats, 2n doubles).  No atomics: the same
 *                    tiles give the same bits as the host loop
 *   bp_plane_blend_fields: bp_plane_blend for tiles (n, fields, tile, tile) of a painter with several label fields:
 *                    field f's tiles tiles[t][f] are blended in tile order into plane f of acc / wsum
 *                    (fields, rows, cols), with the field's own tile means and stds (stats: 2 * n * fields doubles, row
 *                    t * fields + f) where regularise != 0.  One launch over (field, pixel of the bounding box); the
 *                    bits of each plane are bp_plane_blend's on that field's tiles in a contiguous buffer.  BP_EINVAL
 *                    as bp_plane_blend and for fields < 1; BP_EUNSUPPORTED for n * fields * tile^2 >= 2^31 or more
 *                    than 65535 fields.  bp_plane_finish divides all planes at once (count = fields * rows * cols)
 *   bp_plane_finish: out = acc / wsum (IEEE: 0 / 0 = NaN where no tile reaches) */
enum { BP_F64 = 2 }; /* bp_plane_cut's float64 planes (views are BP_F32 / BP_BF16 only) */
size_t bp_plane_cut_workspace(int32_t n, int32_t cut, int32_t tile);
int bp_plane_cut(const void* plane, int32_t dtype, int32_t rows, int32_t cols, const int32_t* origins, int32_t n,
                 int32_t cut, int32_t tile, double* scratch, size_t scratch_bytes, float* out, void* stream);
int bp_plane_blend(const float* tiles, int32_t n, int32_t tile, const int32_t* dst, int32_t bx0, int32_t by0,
                   int32_t bx1, int32_t by1, const double* weight, int32_t regularise, double regularise_std,
                   double* stats, double* acc, double* wsum, int32_t rows, int32_t cols, void* stream);
int bp_plane_blend_fields(const float* tiles, int32_t n, int32_t fields, int32_t tile, const int32_t* dst, int32_t bx0,
                          int32_t by0, int32_t bx1, int32_t by1, const double* weight, int32_t regularise,
                          double regularise_std, double* stats, double* acc, double* wsum, int32_t rows, int32_t cols,
                          void* stream);
int bp_plane_finish(const double* acc, const double* wsum, int64_t count, double* out, void* stream);

/* ---- problematic tiles of a plane (lightcone.paint_plane(return_problematic_tiles=True), process_SLICS.py:212-216) --
 * Which painted tiles hold a pixel more than regularise_std tile standard deviations from the tile mean, how many
 * such pixels, and the offending tiles themselves, on the device between the paint graph and the blend.
 *   bp_tile_outliers: tiles is (n_images, tile, tile) float32; for the (n, fields, tile, tile) tiles of a painter with
 *                    several label fields an image is one (tile, field) pair, row t * fields + f.  One workgroup per
 *                    image: stats[2i] = mean, stats[2i + 1] = population std in float64, by the reduction of
 *                    bp_plane_blend (the same device function: the same bits), and counts[i] (int32) = the number of
 *                    pixels with fabs((double) p - mean) > std * regularise_std, the blend's own expression:
 *                    counts[i] > 0 exactly where bp_plane_blend(regularise = 1) zeroes a weight of image i.  A NaN
 *                    in an image gives a NaN mean and count 0 (every comparison is false, as NumPy's), an infinite
 *                    pixel likewise, a constant image std 0 and count 0.  BP_EINVAL for a null pointer, n_images or
 *                    tile < 1, a regularise_std that is negative or not finite; then BP_EUNSUPPORTED for
 *                    n_images * tile^2 >= 2^31
 *   bp_tile_keep   : tile t of the batch (raw (n, tile, tile) as bp_plane_cut wrote it, painted (n, fields, tile,
 *                    tile), counts (n, fields) from bp_tile_outliers) is problematic if any of its `fields` counts is
 *                    non-zero.  The j-th problematic tile in ascending t takes slot s = *cursor + j; while s < cap:
 *                    kept_index[s] = first_index + t, kept_raw[s] (tile, tile) and kept_painted[s] (fields, tile,
 *                    tile) receive its tiles bit for bit.  Then *cursor += the number of problematic tiles of the
 *                    batch, those beyond cap included.  cursor is one int32 in device memory that the caller zeroes
 *                    once and carries from batch to batch on ONE stream: two ordered launches, the copy, which reads
 *                    it, then the advance.  Slots that are not written stay untouched; cap = 0 only counts.  16-byte
 *                    copies where tile^2 is a multiple of four and raw, painted, kept_raw, kept_painted are 16-byte
 *                    aligned, 4-byte ones otherwise; the bits do not depend on it.  BP_EINVAL for a null raw,
 *                    painted, counts or cursor, null kept_* with cap > 0, n, fields or tile < 1, first_index or
 *                    cap < 0; then BP_EUNSUPPORTED for n * fields * tile^2 >= 2^31, n > 65535 or
 *                    first_index + n >= 2^31
 * Nothing is launched or written on a refusal.  No atomics, no workspace, no host synchronisation: the same inputs
 * give the same bits. */
int bp_tile_outliers(const float* tiles, int32_t n_images, int32_t tile, double regularise_std, double* stats,
                     int32_t* counts, void* stream);
int bp_tile_keep(const float* raw, const float* painted, const int32_t* counts, int32_t n, int32_t fields, int32_t tile,
                 int32_t first_index, int32_t cap, int32_t* cursor, int32_t* kept_index, float* kept_raw,
                 float* kept_painted, void* stream);

/* ---- ensembles of planes and y maps (lightcone.paint_plane_ensemble / paint_light_cone_ensemble) -----------------
 * K draws of a plane are blended into K accumulator pairs (bp_plane_blend_fields with fields = K * F over the
 * (n, K, F, tile, tile) draws of an ensemble graph), K draws of a light cone are projected into K maps; the moments
 * across the K finished planes, or maps, are taken here.
 *   bp_plane_moments: acc and wsum are (draws, count) float64, draw-major; count = fields * rows * cols of a plane or
 *                     res * res of a map.  Per element i: P_k = acc[k][i] / wsum[k][i], or acc[k][i] where wsum is
 *                     NULL; then, in float64 without contraction and in ascending k, bp_paint_store_moments' sums:
 *                     S = ((P_0 + P_1) + ...) + P_{K-1}, M = S / K, Q = ((P_0 - M)^2 + (P_1 - M)^2) + ...,
 *                     mean[i] = M, var[i] = Q / K (the population variance, np.var(ddof=0); two passes, no
 *                     E[P^2] - M^2).  Plain IEEE: 0 / 0 = NaN where no tile reaches, as bp_plane_finish; a NaN or
 *                     infinite draw gives what NumPy gives; draws = 1 gives var = +0 where P_0 is finite.  planes, where
 *                     not NULL, (draws, count), receives the P_k.  One thread owns an element and all its draws, a
 *                     grid-stride loop over count: one launch, no atomics, no workspace, the same inputs give the same
 *                     bits.  Up to 16 quotients stay in registers between the two sums; more are read and divided a
 *                     second time.  16-byte accesses where every pointer is 16-byte aligned and count is even, 8-byte
 *                     ones otherwise; the bits do not depend on either choice.  mean, var and planes must not overlap
 *                     acc or wsum.  With nothing launched or written: BP_EINVAL for a null acc, mean or var, draws < 1
 *                     or count < 1; BP_EUNSUPPORTED for draws > 64.  No host synchronisation. */
int bp_plane_moments(const double* acc, const double* wsum, int32_t draws, int64_t count, double* mean, double* var,
                     double* planes, void* stream);

/* ---- Compton-y map of a light cone (lightcone.project_planes(on_device=True), process_SLICS.py:55-64) -----------
 * A painted plane is resampled to the map's resolution and added into the y map on the device, right behind
 * bp_plane_finish on the same stream: only the finished map comes back.
 *   bp_plane_project_order: y (res, res) float64 += scipy.ndimage.zoom(where(isnan(P), 0, P) * scale, res / n,
 *                     order=order, mode="mirror") for the square float64 plane P (rows == cols == n) and order 2 ... 5,
 *                     in float64: SciPy's B-spline prefilter (its poles and gain; two poles, one after the other, at
 *                     orders 4 and 5) under whole-sample symmetric boundaries along axis 0 then axis 1 (parallel along
 *                     the line: pieces of 224 samples with warm-ups on the mirrored extension that leave <= 1e-18 of
 *                     their start, 32 samples at orders 2 and 3, 64 + 32 at orders 4 and 5, exact to double precision;
 *                     lines shorter than 32 samples take SciPy's closed-form initialisation), then tensor-product
 *                     sampling at i (n - 1) / (res - 1) with order + 1 mirrored taps per axis, one thread per pixel of
 *                     y.  P is not modified.  No atomics: the same inputs give the same bits.  Needs
 *                     bp_plane_project_order_workspace(n, res, order) bytes of `scratch` (two float64 images of the
 *                     plane; 0 for n < 2, res < 2 or an order outside 2 ... 5).  In this order, and with nothing
 *                     launched or written: BP_EINVAL for a null pointer, rows != cols, n < 2 or res < 2;
 *                     BP_EUNSUPPORTED for an order outside 2 ... 5 (orders 0 and 1 have no prefilter and stay on the
 *                     host) and for n * n or res * res >= 2^31; BP_EWORKSPACE for a scratch that is too short.  No
 *                     host synchronisation.
 *   bp_plane_project, bp_plane_project_workspace: the same at order 3. */
size_t bp_plane_project_order_workspace(int32_t n, int32_t res, int32_t order);
int bp_plane_project_order(const double* plane, int32_t rows, int32_t cols, double scale, int32_t order,
                           double* scratch, size_t scratch_bytes, double* y, int32_t res, void* stream);
size_t bp_plane_project_workspace(int32_t n, int32_t res);
int bp_plane_project(const double* plane, int32_t rows, int32_t cols, double scale, double* scratch,
                     size_t scratch_bytes, double* y, int32_t res, void* stream);

/* ---- the low-redshift plane of a light cone (lightcone.paint_small_plane(on_device=True), process_SLICS.py:149-176)
 * ONE tile around a footprint smaller than the network's tile: cut with wrap-around from the periodic mass plane,
 * resampled to the tile, painted, and the footprint cropped from the painted tile, all on one stream.  The window is
 * size x size; its pixel (i, j) is plane[(x0 + i) mod rows, (y0 + j) mod cols] of the rows x cols plane (BP_F32 or
 * BP_F64), the modulo not negative (np.take(mode="wrap")): x0, y0 may be negative or past the edge.  The integers are
 * the host's (lightcone.get_tile's expressions).
 *   bp_window_min  : min_out[0] (device, of the plane's dtype) = the minimum of the window, NaN if the window holds a
 *                    NaN (np.min).  Two stages in a fixed order through `scratch` (bp_window_min_workspace() bytes); the
 *                    value stays on the device.
 *   bp_window_zoom : out (tile, tile) float32 = scipy.ndimage.zoom(w, tile / size, order=3, mode="mirror") of the
 *                    window w -- of w - minimum[0], subtracted in the plane's dtype, where `minimum` (device, of the
 *                    plane's dtype) is not NULL -- in float64 with bp_plane_project's prefilter and sampler, rounded
 *                    once to float32.  size == tile goes through the spline as well.  The first pass gathers from the
 *                    plane; `scratch` is bp_window_zoom_workspace(size, tile) bytes (two float64 images of the window;
 *                    0 for arguments that would be refused).  The plane is not modified.  A window with non-finite
 *                    values is resampled without a fault, but not as SciPy's full-line recursion would spread them.
 *   bp_tile_crop   : out (m, m) float64 = (double) img[(r0 + i) mod tile, (c0 + j) mod tile] of the (tile, tile)
 *                    float32 image: get_tile of a painted tile.
 * In this order, and with nothing launched or written: BP_EINVAL for a null pointer other than `minimum`, rows, cols,
 * size, tile or m < 1, size or tile < 2 in bp_window_zoom, or a dtype that is neither BP_F32 nor BP_F64;
 * BP_EUNSUPPORTED for size^2, tile^2 or m^2 >= 2^31 or an origin of 2^30 or more in absolute value; BP_EWORKSPACE for
 * a scratch that is too short.  No atomics: the same inputs give the same bits.  No host synchronisation. */
size_t bp_window_min_workspace(void);
int bp_window_min(const void* plane, int32_t dtype, int32_t rows, int32_t cols, int32_t x0, int32_t y0, int32_t size,
                  void* scratch, size_t scratch_bytes, void* min_out, void* stream);
size_t bp_window_zoom_workspace(int32_t size, int32_t tile);
int bp_window_zoom(const void* plane, int32_t dtype, int32_t rows, int32_t cols, int32_t x0, int32_t y0, int32_t size,
                   const void* minimum, int32_t tile, double* scratch, size_t scratch_bytes, float* out, void* stream);
int bp_tile_crop(const float* img, int32_t tile, int32_t r0, int32_t c0, int32_t m, double* out, void* stream);

/* ---- fully connected layers of the latent bottleneck (replaces nn.Linear behind nn.Flatten / in front of
 *      nn.Unflatten, utils.py:132-133, 148-157, and their autograd backward) ------------------------------------- */

/* nn.Linear on NHWC views.  A view of logical shape (c, h, w) is read as a row of c*h*w features with c slowest, as
 * torch flattens an NCHW tensor; a flat operand of d features is the view (n, 1, 1, d).  The permutation between that
 * order and NHWC is applied to the activation index inside the kernels; `weight` (out_features, in_features) and its
 * gradient keep torch's layout.  All arithmetic is fp32 (fp32 matrix cores for batches of 32 rows and more, vector ALUs
 * below); every sum has a fixed order, so a call repeated on the same data gives the same bits. */
typedef struct bp_linear {
  int32_t in_features, out_features;
  int32_t in_c, in_h, in_w;    /* logical shape of the input:  in_c * in_h * in_w   == in_features  */
  int32_t out_c, out_h, out_w; /* logical shape of the output: out_c * out_h * out_w == out_features */
  int32_t has_bias;
} bp_linear;

/* Every entry point checks its arguments before launching: views that do not match the descriptor (shape, element
 * type, different batch sizes, n <= 0), a NULL where a pointer is needed or a bias pointer that contradicts has_bias
 * give BP_EINVAL, a short workspace BP_EWORKSPACE; nothing is written then.  Views with cstride != c and coff != 0 are
 * served; channels outside a view are never touched.  No allocation, no synchronisation: capturable.
 *
 * Bytes of partial sums the forward needs for n rows: its sum over in_features is split into slabs over workgroups
 * (the split depends on the layer only, not on n), and a second launch adds the slabs in ascending order.  0 for an
 * invalid descriptor or n <= 0. */
size_t bp_linear_workspace(int32_t n, const bp_linear* desc);

/* y_raw[n][g] = sum_f act(x[n][f]) * weight[g][f] (+ bias[g]).  `x_pw`: the input slot's pending pointwise, applied
 * at load by the channel of feature f (NULL: identity).  The output is RAW: an activation behind the layer stays
 * pending on the output slot's record.  bias non-NULL exactly when desc->has_bias. */
int bp_linear_forward(const bp_linear* desc, const bp_view* x, const bp_pointwise* x_pw, const float* weight,
                      const float* bias, const bp_view* y, void* workspace, size_t workspace_bytes, void* stream);

/* dx[n][f] = sum_g dy[n][g] * weight[g][f]: d(loss)/d(act(x)) from dy = d(loss)/d(y_raw), g ascending. */
int bp_linear_backward_data(const bp_linear* desc, const bp_view* dy, const float* weight, const bp_view* dx,
                            void* stream);

/* dweight[g][f] = sum_n dy[n][g] * act(x[n][f]) and dbias[g] = sum_n dy[n][g], n ascending, each element written once
 * (overwritten, not accumulated).  dbias non-NULL exactly when desc->has_bias. */
int bp_linear_backward_weight(const bp_linear* desc, const bp_view* x, const bp_pointwise* x_pw, const bp_view* dy,
                              float* dweight, float* dbias, void* stream);

/* ---- latent heads: reparametrisation sampler + KL (cvae.py:63-66, 76-77, 126-130) ----------- */
typedef struct bp_latent {
  int32_t n;      /* batch M                         */
  int32_t L;      /* samples per datum (cvae.py:21)  */
  int32_t zc, zh, zw;
  float min_z_var;
} bp_latent;

/* q_raw / p_raw: raw head outputs (N,zh,zw,2*zc) with their pointwise (BN+ReLU); p_raw may be
 * NULL (no prior network: standard-normal prior).  eps: (L,N,zc,zh,zw) standard normal.
 * q_raw NULL (then p_raw must be NULL too): sampling that standard-normal prior (cvae.py:83-85, 97-100): z_mu =
 * z_log_var = 0, so z = eps * (1 + min_z_var), written as that one float32 product; stats4 and kl_sum are zero.  (The
 * reference adds the zero mean, 0 + eps * sd, which turns eps = -0.0 into +0.0; the product keeps -0.0: the one value
 * on which the two differ, and they compare equal.)
 * Outputs: stats4 (4,N,zc,zh,zw) = {z_mu, z_log_var, prior_mu, prior_log_var} (NCHW planes),
 * z (L*N, zh, zw, zc) view, kl_sum: one double = sum[...] of cvae.py:129-130 (un-normalised). */
int bp_latent_forward(const bp_latent* lt, const bp_view* q_raw, const bp_pointwise* q_pw,
                      const bp_view* p_raw, const bp_pointwise* p_pw, const float* eps,
                      float* stats4, const bp_view* z, double* kl_sum, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Gradients w.r.t. the ACTIVATED head outputs (N,zh,zw,2*zc): reparametrisation + KL terms. */
int bp_latent_backward(const bp_latent* lt, const bp_view* dz, const float* stats4,
                       const float* eps, const float* seed /* device scalar dL/dELBO */,
                       float beta_kl, const bp_view* dq_act, const bp_view* dp_act, void* stream);

/* ---- Gaussian log-likelihood head (cvae.py:132-146) ----------------------------------------- */
typedef struct bp_loglik {
  int32_t n;  /* M */
  int32_t L;
  int32_t c, h, w;
  int32_t mu_softplus;  /* last activation of the mean head: 1 softplus, 0 none */
  int32_t predict_var;
  float alpha_var, beta_kl, likelihood_scaling;
} bp_loglik;

/* x: NCHW (M,c,H,W); mu_raw / var_raw: (L*M,H,W,c) raw head outputs with optional pointwise.
 * Writes x_mu (NCHW, L*M) [and x_log_var], and stats (floats):
 *   [0]=ELBO [1]=KL_term [2..2+c)=log_likelihood [..+c)=fixed_var [..+c)=free_var. */
size_t bp_loglik_workspace(const bp_loglik* ll);
int bp_loglik_forward(const bp_loglik* ll, const float* x_nchw, const bp_view* mu_raw,
                      const bp_view* var_raw, const double* kl_sum, float* x_mu_nchw,
                      float* x_log_var_nchw, float* stats, void* workspace,
                      size_t workspace_bytes, void* stream);
/* d(seed*ELBO)/d(mu_raw), d/d(var_raw). */
int bp_loglik_backward(const bp_loglik* ll, const float* x_nchw, const bp_view* mu_raw,
                       const bp_view* var_raw, const float* seed, const bp_view* d_mu_raw,
                       const bp_view* d_var_raw, void* stream);

/* ---- scoring a painter on held-out tiles (CVAE.score, CVAEPainter.score) ------ */
/* Per-SAMPLE Gaussian log-density of the truth under the two heads, in float64:
 *   out[(l n + m) c + ch] = sum_{y,x} [ -log(2 pi)/2 - lv/2 - (x - x_mu)^2 exp(-lv) / 2 ]
 * for sample l n + m of mu_raw / var_raw against x[m].  x_mu is the float32 value the paint paths read from the mean
 * head (softplus_f(raw) with ll->mu_softplus, bp_view_to_nchw's device function), lv the variance head's output, 0 for
 * var_raw == NULL; every other operation is float64 without contraction: d = (double) x - (double) x_mu,
 * term = (c0 - 0.5 lv) - (0.5 (d d)) exp(-lv).  Only n, L, c, h, w and mu_softplus of `ll` are read.
 *   x_nchw : (n, c, H, W) float32;   mu_raw, var_raw : (L n, H, W, c) fp32 views, any cstride / coff
 *   out    : (L n, c) float64;       workspace : bp_loglik_samples_workspace(ll) bytes
 * One streaming launch over samples x chunks of 2048 pixels plus one small launch that adds a sample's chunk sums in
 * a fixed order; x, mu and var are each read once, 16 bytes per lane where c == cstride == 1, H W % 4 == 0 and the
 * pointers are 16-byte aligned, one float per access otherwise.  How a sample's pixels are split into partial sums
 * depends on (h, w, c) alone: no atomics, the same inputs give the same bits, and a sample's sum has the same bits
 * whatever else is in the launch.  Non-finite values get no special handling: a NaN in one sample is that sample's.
 * Before anything is written: BP_EINVAL for a null pointer other than var_raw, a malformed view, n, L, c, h or w < 1,
 * mu_raw->n != n L or view shapes that disagree with `ll`; then BP_EUNSUPPORTED for a bf16 view, L > 64 or
 * n L H W c >= 2^31; then BP_EWORKSPACE.  bp_loglik_samples_workspace returns 0 for a descriptor that would be refused. */
size_t bp_loglik_samples_workspace(const bp_loglik* ll);
int bp_loglik_samples(const bp_loglik* ll, const float* x_nchw, const bp_view* mu_raw, const bp_view* var_raw,
                      double* out, void* workspace, size_t workspace_bytes, void* stream);
/* The score of each tile from its K = lt->L draws: with s(lv) = exp(lv / 2) + min_z_var in float64 from the float32
 * stats4 planes of bp_latent_forward and eps (L, n, zc, zh, zw), for tile m and draw k, over the latent elements j
 * (64 at a time by a fixed shuffle tree, the groups in ascending order),
 *   r_k     = sum_j [ (log s_q - log s_p) + (eps^2/2 - ((z_mu + eps s_q - p_mu) / s_p)^2 / 2) ]
 *   log w_k = ((loglik[(k n + m) c + 0] + ...) + loglik[.. + c - 1]) + r_k
 *   score[m] = { logsumexp_k(log w_k) - log K,  mean_k log w_k,  mean_k sum_c loglik,  -mean_k r_k,
 *                exp(2 lse(log w) - lse(2 log w)) }          (bound, elbo, log_likelihood, kl, ess)
 * logsumexp subtracts the maximum; a tile whose log w_k are all -inf gets bound = -inf and ess = NaN; K = 1 gives
 * bound == elbo bit for bit and ess == 1.  A model without prior network passes zero prior planes in stats4 (what
 * bp_latent_forward writes), so s_p = 1 + min_z_var.  log_w: NULL or (L, n), receives every log w_k.
 * One launch, one wave per tile, lane k takes draws k (no atomics, no workspace, no host synchronisation).  Before
 * anything is written: BP_EINVAL for a null pointer other than log_w or n, L, c or a latent extent < 1; then
 * BP_EUNSUPPORTED for L > 64. */
int bp_posterior_score(const bp_latent* lt, const float* stats4, const float* eps, const double* loglik, int32_t c,
                       double* score, double* log_w, void* stream);

/* ---- GAN heads (the CGAN of trained_models/README.md:95-144; no code in the reference) ------ */
/* out = f(act(in)), kind 0 identity, 1 tanh (generator output, README.md:128), 2 sigmoid, 3 softplus.  Also the
 * saturating layers of the CVAE's layer language (models/utils.py:68-73, 140-145; graph.UnaryUnit).  With
 * v = act(in) = the pointwise of `pw` (NULL: v = in), all in float32:
 *   kind 1: tanhf(v)    kind 2: 1 / (1 + expf(-v))    kind 3: v > 20 ? v : log1pf(expf(v))  (torch.nn.Softplus(1, 20))
 * bp_unary_backward: d_in = (dout + dout2) * f'(y) from the SAVED OUTPUT y = f(v) alone (dout2 may be NULL):
 *   kind 0: 1    kind 1: 1 - y*y    kind 2: y * (1 - y)    kind 3: -expm1f(-y)  (= sigmoid(v); 1 above the threshold)
 * d_in is d(loss)/d(act(in)): the producer of `in` applies its own activation derivative.  d_in may be dout.
 * Views of one grid (n, h, w, c), channel slices of wider buffers included; nothing outside [coff, coff + c) is
 * written.  Each lane moves 16 bytes where every view allows it (c, cstride, coff multiples of 4, or all views dense,
 * and 16-byte aligned bases); any other view runs one element per thread with the same arithmetic per element.  No
 * atomics, no workspace, no host synchronisation.  fp32 views only: BP_EUNSUPPORTED (nothing written) for a bf16 view;
 * BP_EINVAL for views that are not one grid or a kind outside 0..3. */
int bp_unary_forward(const bp_view* in, const bp_pointwise* pw, int32_t kind, const bp_view* out,
                     void* stream);
int bp_unary_backward(const bp_view* dout, const bp_view* dout2, const bp_view* y, int32_t kind,
                      const bp_view* d_in, void* stream);
/* sum over samples [n0,n1) of BCE(sigmoid(raw), target) evaluated on the logits; and its gradient
 * d_raw = scale * (sigmoid(raw) - target) for those samples. */
int bp_bce_logits(const bp_view* raw, int32_t n0, int32_t n1, float target, double* sum,
                  void* workspace, size_t workspace_bytes, void* stream);
int bp_bce_logits_grad(const bp_view* raw, int32_t n0, int32_t n1, float target, float scale,
                       const bp_view* d_raw, void* stream);
/* sum |fake - x| ; d_raw = (d_fake + l1_scale*sign(fake - x)) * (1 - fake^2) through the Tanh. */
int bp_l1_sum(const bp_view* fake, const float* x_nchw, double* sum, void* workspace,
              size_t workspace_bytes, void* stream);
int bp_tanh_l1_backward(const bp_view* fake, const float* x_nchw, const bp_view* d_fake,
                        float l1_scale, const bp_view* d_raw, void* stream);

/* ---- device-side batch assembly (replaces BAHAMASDataset.get_stack + transform on the host,
 *      utils/datasets.py:305-404): the stacks live in HBM, one launch builds a field of a batch.
 * desc100/desc150: n records {const float* base; int32 pitch; int32 r0,rr,rc,c0,cr,cc; int32 pad}
 *   (source row = r0 + rr*r + rc*c, col = c0 + cr*r + cc*c: the dihedral tile permutation);
 * xform: n records {double scale, inv_sigma, inv_k; int32 mode; int32 pad}, mode 1 = shift-log.
 * out: (n,1,tile,tile) float32 = transform(scale * (tile100 + tile150)). */
int bp_gather_tiles(const void* desc100, const void* desc150, const void* xform, int32_t n,
                    int32_t tile, float* out_nchw, void* stream);
/* Training sets built with subtract_minimum (datasets.py:398-403, the SLICS_density convention) and / or a
 * split-scale transform, from the same descriptors:
 *   bp_tile_minima        : minima[i] (device, n float32) = min over the tile of the float32 value scale * (tile100 +
 *                           tile150) that bp_gather_tiles forms in front of its transform; NaN if the tile holds a NaN
 *                           (np.min).  One workgroup per tile: lanes, waves, LDS.  min is exact: bit-equal to the host.
 *   bp_gather_tiles_scales: out (n, levels, tile, tile) float32 NCHW planes, levels = n_scale + include_original, in
 *                           bp_split_scale's channel order = the pyramid of the float32 tile
 *                           transform(scale * (tile100 + tile150) [- minima[i]]) (`minima` may be NULL: nothing is
 *                           subtracted; the subtraction is a float32 one, `d -= d.min()`).  The tile is the value
 *                           bp_gather_tiles stores and the pyramid is bp_split_scale's, bit for bit; weights, radii as
 *                           for bp_split_scale; n_scale = 1 stores the tile itself (twice with include_original) and
 *                           needs no scratch.  The gather runs inside the axis-0 pass of the coarsest level: the
 *                           stacks are read once.  scratch: bp_gather_tiles_scales_workspace(n, tile, n_scale) bytes.
 * bp_split_scale's limits (r <= 96, <= 16 scales, n <= 65535) and error order: BP_EINVAL / BP_EUNSUPPORTED /
 * BP_EWORKSPACE are returned before anything is written.  No atomics, no host synchronisation. */
int bp_tile_minima(const void* desc100, const void* desc150, const void* xform, int32_t n, int32_t tile,
                   float* minima, void* stream);
size_t bp_gather_tiles_scales_workspace(int32_t n, int32_t tile, int32_t n_scale);
int bp_gather_tiles_scales(const void* desc100, const void* desc150, const void* xform, const float* minima,
                           int32_t n, int32_t tile, int32_t n_scale, int32_t include_original, const double* weights,
                           const int32_t* radii, void* scratch, size_t scratch_bytes, float* out_nchw, void* stream);
/* bp_gather_tiles_scales with range-compression mode `mode` over `records` (see bp_paint_load_mode) in place of the
 * transform xform names: xform's `scale` is still applied, its mode / inv_sigma / inv_k are not read.  With n_scale = 1,
 * include_original = 0 and minima = NULL this is bp_gather_tiles for any mode (out (n, 1, tile, tile)). */
int bp_gather_tiles_scales_mode(int32_t mode, const double* records, const void* desc100, const void* desc150,
                                const void* xform, const float* minima, int32_t n, int32_t tile, int32_t n_scale,
                                int32_t include_original, const double* weights, const int32_t* radii, void* scratch,
                                size_t scratch_bytes, float* out_nchw, void* stream);
/* The CGAN's training batch in ONE launch, written straight into the inputs of its training plan (models/cgan.py).
 * in100 / in150 / in_xform and lab100 / lab150 / lab_xform: bp_gather_tiles' records of the input field (dm) and of the
 * label field (pressure); of the xform records only `scale` is read.  in_minima: NULL, or the bp_tile_minima of the input
 * field, subtracted in float32 in front of the transform (subtract_minimum sets).  cam: (n, 2, 3) float64, the rows
 * {sigma, k0, k1} of the input field and then of the label field.  aux: n float32, the conditioning value z - 1.
 * A pixel is  (float) (log((double) s / sigma + 1) / k0 - k1),  s = scale * (tile100 + tile150) [- minimum]: the value
 * bp_gather_tiles forms at mode 0 under bp_paint_load_cam's transform, bit for bit (one shared device function).
 * Destinations, all (n, tile, tile) fp32 views:
 *   gen_in      c = 2: [dm, aux]             the generator's input
 *   d_real      c = 3: [dm, aux, pressure]   the real half of the discriminator's input
 *   d_fake_cond c = 2: [dm, aux]             the conditioning channels of the fake half
 *   x_nchw      (n, 1, tile, tile) dense     pressure, as bp_l1_sum and bp_tanh_l1_backward read it
 * Only the named channels are written: the bytes between coff + c and cstride of a pixel (a pad channel, the fake half's
 * pressure channel) are left alone.  Every stack value is read once; dm is stored three times, pressure twice.  A lane
 * owns four consecutive pixels of a row: 16-byte stores where a destination is dense and aligned, 8- and 4-byte stores
 * with the same values otherwise.  Any tile >= 1 with tile^2 < 2^31, any n >= 1, 64-bit addressing of the destinations.
 * No atomics, no workspace, no host synchronisation.  Before anything is written: BP_EINVAL for a NULL argument other
 * than in_minima, n <= 0, tile <= 0, a view that is not (n, tile, tile) or has another channel count; BP_EUNSUPPORTED for
 * a bf16 view. */
int bp_gather_tiles_gan(const void* in100, const void* in150, const void* in_xform, const float* in_minima,
                        const void* lab100, const void* lab150, const void* lab_xform, const double* cam,
                        const float* aux, int32_t n, int32_t tile, const bp_view* gen_in, const bp_view* d_real,
                        const bp_view* d_fake_cond, float* x_nchw, void* stream);

/* ---- optimiser (replaces torch.optim.Adam.step, painter.py:93,228; same arithmetic) --------- */
int bp_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                 float lr, float beta1, float beta2, float eps, int32_t step, void* stream);
/* The same update with its scalars read from device memory - hyper[6] = {lr, beta1, beta2, eps,
 * 1 - beta1^step, sqrt(1 - beta2^step)} - so that the launch can sit in a captured hipGraph of the whole
 * training step while the learning rate and the step number keep changing. */
int bp_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                     const float* hyper, void* stream);

/* ---- data parallel: small-message all-reduce over peer memory (csrc/peer_comm.hip) --------------------------
 * The reference is single-device; sharding its minibatch keeps its arithmetic only if every BatchNorm2d sees the
 * statistics of the GLOBAL batch (painter.py:224 feeds the whole minibatch through the module): 44 dependent all-reduces
 * of <= 2 KB per step.  One process per GPU; each rank calls bp_peer_create (allocates its fine-grained exchange buffer,
 * returns an opaque communicator and an IPC handle of bp_peer_handle_bytes() bytes), the host exchanges the handles
 * (any transport: torch.distributed all_gather), each rank passes the world_size handles, in rank order, to bp_peer_open.
 * bp_peer_all_reduce then sums `n` (<= bp_peer_max_doubles()) doubles in place over the ranks with ONE kernel on `stream`:
 * peer stores over xGMI, per-rank flags, a fixed rank-order sum (bitwise the same result on every rank).  Every rank must
 * issue the same sequence of calls.  Spins are bounded (`spin_limit` polls, <= 0: default): a timeout is counted in the
 * communicator's status word (bp_peer_status, synchronising) and the call's result is then undefined. */
int bp_peer_handle_bytes(void);
int bp_peer_max_doubles(void);
int bp_peer_slots(void);                 /* slots of the exchange ring: a step must issue fewer than half as many collectives */
int bp_peer_create(int rank, int world, void** comm_out, void* handle_out);
int bp_peer_open(void* comm, const void* handles);
int bp_peer_all_reduce(void* comm, double* data, int n, int64_t spin_limit, void* stream);
int64_t bp_peer_status(void* comm);
/* Bind `comm` (NULL: unbind) to the CALLING host thread.  While bound, every launch that finishes a layer's batch-norm
 * statistics together with the finalize arithmetic -- bp_conv_forward_bn (the `count` of bp_bn_train is then the GLOBAL
 * pixel count) and bp_act_backward_bn (`count` global, `pscale` = 1 / world size) -- exchanges each channel's two sums with
 * the other ranks inside that kernel, in place of a separate all-reduce: the collective number advances as in
 * bp_peer_all_reduce, so every rank must issue the same sequence of both kinds of call (cvae.py:224 semantics: the
 * statistics of the global batch, as one nn.BatchNorm2d over the whole minibatch computes them). */
int bp_peer_bind(void* comm);
/* The per-channel exchange of the bound form on its own, one collective: data[ch] and data[c + ch] (2 c <=
 * bp_peer_max_doubles()) summed over the ranks by workgroup ch -- the start-up self-test of that path (dist.py). */
int bp_peer_exchange_check(void* comm, double* data, int c, void* stream);
int bp_peer_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* BP_HIP_H */
